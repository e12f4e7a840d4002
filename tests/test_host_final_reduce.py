"""The host side of the record mode (pinot_amd/csrc/host_final.h) without a GPU: a stand-alone program with its own
main (tests/host_final/reduce_main.cpp), built from the reducer header alone with AddressSanitizer and UBSan and run
as a fresh process.

reduce: full sets of valid records, a word still carrying the previous tag, a word never written (tag 0), an accumulator
with a new low and an old high word, K = 0 and K at the record's limit -- accept versus not-yet, the int64 totals, and
the double totals against a straight restatement of the device's lane-strided and butterfly order over doubles that
include NaN, -0.0 and infinities.

table: the plan-time block table and the shared range arithmetic (tile_range.h). The program prints, this file
compares: for total_work 0..200, a few grids and both walks every tile belongs to exactly one wave range, a block's
range is its waves' ranges end to end, and its segment span equals a brute-force count."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host_final", "reduce_main.cpp")
CLANG = "/opt/rocm/lib/llvm/bin/clang++"
ENTRY_LENGTHS = (1, 3, 2, 9, 1, 1, 17, 4)  # tiles per work-list entry, cyclically


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = CLANG if os.path.exists(CLANG) else (shutil.which("clang++") or shutil.which("g++"))
    assert cxx, "no C++ compiler"
    exe = str(tmp_path_factory.mktemp("host_final") / "reduce_main")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-ffp-contract=off",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", exe, SRC])
    return exe


def _run(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=300)


def test_record_reducer(program):
    p = _run(program, "reduce")
    assert p.returncode == 0 and "REDUCE OK" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]


def _entry_begins(total):
    out, t, i = [], 0, 0
    while t < total or not out:
        out.append(t)
        t += ENTRY_LENGTHS[i % len(ENTRY_LENGTHS)]
        i += 1
    return out


def test_block_table(program):
    p = _run(program, "table", ",".join(str(x) for x in ENTRY_LENGTHS))
    assert p.returncode == 0, p.stderr[-3000:]
    cases, cur = [], None
    for line in p.stdout.splitlines():
        f = line.split()
        if f[0] == "T":
            cur = (int(f[1]), int(f[2]), int(f[3]), [])
            cases.append(cur)
        else:
            cur[3].append([int(x) for x in f[1:]])
    assert len(cases) == 7 * 201
    for walk, nblocks, total, blocks in cases:
        assert len(blocks) == nblocks
        begins = _entry_begins(total)
        owner = [0] * total
        entry = [max(e for e, t0 in enumerate(begins) if t0 <= t) for t in range(total)]
        for b, bb, be, first, k, *waves in blocks:
            ranges = list(zip(waves[0::2], waves[1::2]))
            assert len(ranges) == 4
            for lo, hi in ranges:
                assert 0 <= lo <= hi <= total, (walk, nblocks, total, b)
                for t in range(lo, hi):
                    owner[t] += 1
            # the block's range: its waves' ranges end to end
            assert ranges[0][0] == bb and ranges[-1][1] == be, (walk, nblocks, total, b)
            assert all(ranges[i][1] == ranges[i + 1][0] for i in range(3)), (walk, nblocks, total, b)
            if walk == 2:  # an XCD's workgroups stay inside its eighth of the work list
                x = b & 7
                assert total * x // 8 <= bb and be <= total * (x + 1) // 8, (walk, nblocks, total, b)
            # brute force: the entries holding the block's tiles (a tile belongs to the last entry beginning at or before it)
            touched = sorted({entry[t] for t in range(bb, be)})
            assert k == len(touched), (walk, nblocks, total, b, k, touched)
            if touched:
                assert first == touched[0] and touched == list(range(first, first + k)), (walk, nblocks, total, b)
        assert all(c == 1 for c in owner), (walk, nblocks, total)
