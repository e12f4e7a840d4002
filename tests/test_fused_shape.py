"""The launch shape of small fused scans (pinot_amd/csrc/fused_shape.h) without a GPU: a stand-alone program with its
own main (tests/fused_shape/shape_main.cpp), built from the header alone with AddressSanitizer and UBSan and run as a
fresh process.

sweep: tile counts 1..8192 (every count below 300, then every 7th), ring slots of 512 B..19 KB in both modes, 1 and 256
CUs. Asserted per input: blocks * 4 * T >= tiles; the chosen LDS times the chosen workgroups per CU fits 160 KiB; all
blocks resident at once; one slot for one-tile waves, at least two for T >= 2 whenever two fit; T the smallest of its
mode and of both modes (brute force), the streamed mode on a tie; a forced ring depth is kept.

The two pinned cases are the headline's sorted SSB Q1.2 and Q1.3, derived by hand below."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "fused_shape", "shape_main.cpp")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"

# Both queries filter LO_DISCOUNT (11 values: 4 bit planes) and LO_QUANTITY (50 values: 6 planes) beside the sorted
# LO_ORDERDATE range, which stages nothing. Every staged region carries 16 guard bytes on both sides.
#   deferred slot: 4 * 256 + 32 + 6 * 256 + 32                     = 2624 B; doc rings 4 waves * 4 B * 512  = 8192 B
#   streamed slot: 2624 + LO_EXTENDEDPRICE's packed values 24 * 256 + 32
#                       + LO_DISCOUNT's packed ids 4 * 256 + 32     = 9856 B; doc rings 4 waves * 2 B * 512  = 4096 B
# LDS of a workgroup = 4 waves * nbuf * slot + doc rings + 448 B static; a CU has 163840 B and admits 5 workgroups.
DEFER = (2624, 8192)
STREAM = (9856, 4096)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = CLANG if os.path.exists(CLANG) else (shutil.which("clang++") or shutil.which("g++"))
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp("fused_shape") / "shape_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-o", exe, SRC])
    return exe


def _one(exe, tiles, cus=256, nbuf=0, stream=STREAM, defer=DEFER):
    p = subprocess.run([exe, "one", str(tiles), *map(str, stream + defer), str(cus), str(nbuf)], capture_output=True,
                       text=True, timeout=60)
    assert p.returncode == 0, p.stderr[-3000:]
    mode, blocks, nbuf, bpc, t = (int(x) for x in p.stdout.split())
    return {"mode": mode, "blocks": blocks, "nbuf": nbuf, "bpc": bpc, "T": t}


def test_shape_sweep(program):
    p = subprocess.run([program, "sweep"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "SHAPE OK" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]
    assert int(p.stdout.split()[-1]) > 50_000


def test_shape_q12(program):
    """Sorted SSB Q1.2: 3776 tiles on 256 CUs.
    Deferred, T = 1: 944 workgroups need 4 per CU (1024 >= 944 > 768), so at most 163840 // 4 = 40960 B each: three
    slots 4 * 3 * 2624 + 8192 + 448 = 40128 B fit, four (50624 B) do not.
    Streamed, T = 1: 944 workgroups; one slot: 4 * 9856 + 4096 + 448 = 43968 B, 3 per CU: 768 < 944. T = 2: 472 workgroups,
    two slots 83392 B, 1 per CU: 256 < 472. T = 3: 315 workgroups, 1 per CU at two slots or more, 256 < 315.
    T = 4: 236 workgroups, four slots 4 * 4 * 9856 + 4544 = 162240 B <= 163840, 1 per CU: 256 >= 236, fits; five do not.
    T 1 < 4: the deferred mode."""
    assert _one(program, 3776) == {"mode": 1, "blocks": 944, "nbuf": 3, "bpc": 4, "T": 1}
    assert _one(program, 3776, defer=(0, 0)) == {"mode": 0, "blocks": 236, "nbuf": 4, "bpc": 1, "T": 4}


def test_shape_q13(program):
    """Sorted SSB Q1.3: 854 tiles on 256 CUs. Its week is too sparse for the density rule to stream LO_EXTENDEDPRICE's
    24 bits: the streamed slot adds LO_DISCOUNT's packed ids alone, 2624 + 4 * 256 + 32 = 3680 B (PHIP_SHAPE_TRACE=1 on the
    SF100 segments prints these inputs). T = 1 needs 214 workgroups, fewer than the CUs, so one per CU is enough and the
    ring takes what a CU's LDS holds: eight slots, 4 * 8 * 3680 + 4096 + 448 = 122304 B <= 163840. Deferred fits T = 1
    as well: a tie, the density rule's mode (streamed) stays -- the shape the plan had before the rule."""
    assert _one(program, 854, stream=(3680, 4096)) == {"mode": 0, "blocks": 214, "nbuf": 8, "bpc": 1, "T": 1}
    assert _one(program, 854, stream=DEFER, defer=(0, 0)) == {"mode": 0, "blocks": 214, "nbuf": 8, "bpc": 1, "T": 1}


def test_shape_one_cu(program):
    """One CU, 40 tiles, the deferred slot, ring depth forced to 1: T = 1 needs 10 workgroups, 5 fit; T = 2 needs 5.
    Unforced, T = 2 takes two slots: 4 * 2 * 2624 + 8640 = 29632 B, 5 per CU still."""
    assert _one(program, 40, cus=1, nbuf=1, stream=DEFER, defer=(0, 0)) == {"mode": 0, "blocks": 5, "nbuf": 1, "bpc": 5, "T": 2}
    assert _one(program, 40, cus=1, stream=DEFER, defer=(0, 0)) == {"mode": 0, "blocks": 5, "nbuf": 2, "bpc": 5, "T": 2}
