"""Digest of ONE lone augmented factorisation (N = n + 1, nf = n; default n = 16384) of a seeded matrix, to compare two builds bit by bit:
    python tools/r08/dump_augmented_factor.py [n] > factor_digest.txt
prints the SHA-256 of the lower triangle of the first nf rows (the factor), the tail row and the corner as hex floats, and logdet."""
import hashlib, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch
from gpar_amd import hip

n = int(sys.argv[1]) if len(sys.argv) > 1 else 16384
N = n + 1
dev = torch.device("cuda:0")
g = torch.Generator(device="cpu").manual_seed(n)
B = torch.randn(N, 64, dtype=torch.float64, generator=g).to(dev)
A = hip.alloc_matrix(N, N, dev)
A.copy_(B @ B.T / 64.0)
A.diagonal().add_(1.0)
del B
logdet, info = hip.potrf_(A, n)
assert int(info.item()) == 0
L = torch.tril(A[:n, :n]).cpu().numpy()
tail = A[n, :n].cpu().numpy()
print(f"n {n}")
print("factor", hashlib.sha256(L.tobytes()).hexdigest())
print("tail_row", hashlib.sha256(tail.tobytes()).hexdigest(), "sum", float(tail.sum()).hex())
print("corner", float(A[n, n]).hex(), "logdet", float(logdet).hex())
