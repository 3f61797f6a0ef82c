"""The factorisation schedule as data (gpar_amd/csrc/potrf_schedule.h), checked without a GPU through its printer
(tools/potrf_schedule.cpp): structural facts every schedule must satisfy, over a sweep of shapes, and the property potrf_exec's
bit-for-bit guarantee rests on - the description of the steps does not depend on the look-ahead setting."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = re.compile(r"^step \[(\d+),(\d+)\) (\S+) G=(\d+) update (none|one|slice\+rest)(?: \[(\d+),(\d+)\) (gemm|small)(\+tail)?)?"
                  r"(?: rest \[(\d+),(\d+)\)(\+tail)?)?$")
UNFUSED = 2   # GPAR_POTRF_UNFUSED


def _shapes():
    """(N, nf, lda, batch, flags): the augmented matrices (n + 1, n) of the log marginal likelihood for n = 100 .. 20011 - every 7th
    n, the sizes the benchmarks and the parity suites use, and every n around the multiples of 512 -, matrices without a tail, with
    tails of 2, 16, 17 and 50 rows (17: just over the tail split's limit; 50: a posterior's appended rows), ragged nf, odd lda."""
    ns = set(range(100, 20012, 7)) | {100, 512, 1300, 2048, 4096, 5200, 5632, 6656, 8192, 12288, 16384, 20011}
    for c in range(512, 20012, 512):
        ns.update(range(c - 3, c + 4))
    shapes = []
    for batch in (1, 4, 16):
        for flags in (0, UNFUSED):
            for n in sorted(ns):
                shapes.append((n + 1, n, n + 1 + (n + 1) % 2 + (n % 11 == 0), batch, flags))   # (every 11th: an odd lda)
            for n in range(100, 20012, 331):
                for tail in (0, 2, 16, 17, 50):
                    shapes.append((n + tail, n, n + tail + (n + tail) % 2, batch, flags))
    return shapes


@pytest.fixture(scope="module")
def printer(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("potrf_schedule") / "potrf_schedule")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")   # the compiler build() uses
    subprocess.check_call([hipcc, "-std=c++17", "-O1", os.path.join(ROOT, "tools", "potrf_schedule.cpp"), "-o", exe])
    return exe


def _run(exe, shapes, **env):
    e = {k: v for k, v in os.environ.items() if not k.startswith(("GPAR_POTRF_", "GPAR_PANEL_"))}
    e.update(env)
    text = "".join("%d %d %d %d %d\n" % s for s in shapes)
    return subprocess.run([exe], input=text, env=e, check=True, capture_output=True, text=True).stdout.splitlines()


def _parse(lines):
    """-> [(shape dict, policy dict, [step tuples])]"""
    out = []
    for line in lines:
        if line.startswith("shape "):
            out.append((dict((k, int(v)) for k, v in (f.split("=") for f in line.split()[1:])), {}, []))
        elif line.startswith("policy "):
            out[-1][1].clear()   # (a batch that is not lock-step: the lone schedule's policy replaces it)
            out[-1][1].update((k, int(v)) for k, v in (f.split("=") for f in line.split()[1:]))
        elif line.startswith("not lock-step"):
            out[-1][0]["batch"] = 1
        else:
            m = STEP.match(line)
            assert m, line
            out[-1][2].append(m.groups())
    return out


def _ceil_div(a, b):
    return -(-a // b)


def test_every_schedule_tiles_the_columns_and_updates_every_trailing_element_once(printer):
    shapes = _shapes()
    parsed = _parse(_run(printer, shapes))
    assert len(parsed) == len(shapes)
    seen = set()
    for (sh, pol, steps), given in zip(parsed, shapes):
        N, nf, batch = sh["N"], sh["nf"], sh["batch"]
        assert (N, nf, sh["lda"]) == given[:3] and batch in (1, given[3])
        assert steps, sh
        col = 0
        for k0, kend, form, G, update, s0, s1, kind, stail, r0, r1, rtail in steps:
            k0, kend, G = int(k0), int(kend), int(G)
            seen.add(form)
            # the steps tile [0, nf) exactly and in order
            assert k0 == col and k0 < kend <= nf, (sh, k0, kend)
            col = kend
            if form == "grouped":
                assert k0 > 0 and G == pol["group"] and kend - k0 == G * pol["nbo"], (sh, k0)
            elif form == "fused-group":
                assert 2 <= G <= pol["fuse_max"] and kend - k0 == G * pol["nbo"], (sh, k0)
            else:
                assert G == 1
            # rows left below the step: [kend, N) is updated exactly once, slice and rest partition it
            if kend >= N:
                assert update == "none"
                continue
            assert update != "none", (sh, k0)
            s0, s1 = int(s0), int(s1)
            assert s0 == kend and s0 < s1 <= N, (sh, k0)
            if update == "one":
                assert s1 == N and r0 is None, (sh, k0)
            else:
                assert (int(r0), int(r1)) == (s1, N) and s1 < N, (sh, k0)
            # a tail-split piece only in a lock-step batch with 1 .. 16 augmented rows, and only where it removes a tile row
            for start, tail in ((s0, stail), (s1, rtail)):
                if tail:
                    assert batch > 1 and 0 < N - nf <= 16, (sh, k0)
                    assert start < nf and _ceil_div(N - start, 128) > _ceil_div(nf - start, 128), (sh, k0, start)
                elif batch > 1 and 0 < N - nf <= 16 and start < nf and not (start == s0 and kind == "small") and \
                        not (start == s1 and update == "one"):
                    assert _ceil_div(N - start, 128) == _ceil_div(nf - start, 128), (sh, k0, start)
            if kind == "small":
                assert kend < nf and (s1 - s0) % 64 == 0 and (kend - k0) % 64 == 0 and not stail, (sh, k0)
        assert col == nf, sh
    assert seen == {"grouped", "fused-group", "fused", "leaf-batch", "leaf"}, seen   # the sweep reaches every panel form


def test_the_steps_do_not_depend_on_the_look_ahead_setting(printer):
    shapes = _shapes()
    off = _run(printer, shapes, GPAR_POTRF_LOOKAHEAD="0")
    on = _run(printer, shapes, GPAR_POTRF_LOOKAHEAD="1")
    default = _run(printer, shapes)
    assert any(line.startswith("policy lookahead=1") for line in on) and any(line.startswith("policy lookahead=0") for line in off)

    def steps(lines):
        return [line if not line.startswith("policy ") else re.sub(r"lookahead=\d+ ", "", line) for line in lines]

    assert steps(off) == steps(on) == steps(default)
    assert any(line.startswith("step ") for line in off)
