"""CPU checks of the fc data gradient's W-in-registers kernel (csrc/fc_gemm.hip,
fc_dgrad_wreg_kernel): its work map and its LDS swizzle.

The map (csrc/work_map.h, fc_dgrad_map) is the function the kernel itself calls; it needs no HIP
header, so a small host program prints it here. For every R the (row slot, 32-column unit) cells
of da3 must be owned by exactly one (block, wave), no block may walk past ceil(R / 64) row slots,
and the 13 blocks of a stream must sit on consecutive positions of one XCD unless the stream
straddles the end of an XCD's blocks. The swizzle is checked with the bank model of
scripts/lds_conflicts.py on the byte addresses the kernel's B-fragment reads use.
"""
import importlib.util
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("lds_conflicts", os.path.join(ROOT, "scripts", "lds_conflicts.py"))
lds = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(lds)

STREAMS, SLICES, BLOCKS, COLS = 19, 13, 247, 3136
ROWS = [1, 21, 64, 65, 1215, 1216, 1217, 3653, 413696]

_SRC = r"""
#include <cstdio>
#include <cstdlib>
#include "work_map.h"
int main(int argc, char** argv) {
    std::printf("%d %d %d %d %d %d\n", fi::kDgStreams, fi::kDgSlices, fi::kDgBlocks, fi::kDgSlotRows,
                fi::kDgSliceCols, fi::kDgWaveCols);
    for (int a = 1; a < argc; ++a)
        for (int b = 0; b < fi::kDgBlocks; ++b) {
            const fi::FcDgradMap m = fi::fc_dgrad_map(b, std::atoi(argv[a]));
            std::printf("%s %d %d %d %d %d %d\n", argv[a], b, m.stream, m.slice, m.nslots, m.xcd, m.pos);
        }
    return 0;
}
"""


@pytest.fixture(scope="module")
def maps(tmp_path_factory):
    d = tmp_path_factory.mktemp("fc_dgrad_map")
    src, exe = d / "map.cpp", d / "map"
    src.write_text(_SRC)
    subprocess.run(["g++", "-std=c++17", "-O1", "-I", os.path.join(ROOT, "freeimpala_amd", "csrc"), str(src),
                    "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)] + [str(r) for r in ROWS], capture_output=True, text=True, check=True).stdout
    lines = out.splitlines()
    assert [int(v) for v in lines[0].split()] == [STREAMS, SLICES, BLOCKS, 64, 256, 32]
    per = {r: [] for r in ROWS}
    for ln in lines[1:]:
        r, b, stream, sl, nslots, xcd, pos = (int(v) for v in ln.split())
        per[r].append(dict(block=b, stream=stream, slice=sl, nslots=nslots, xcd=xcd, pos=pos))
    return per


def _slots(m):
    """row slots the kernel's loop walks for a block: stream, stream + 19, ... < nslots"""
    return range(m["stream"], m["nslots"], STREAMS)


@pytest.mark.parametrize("R", ROWS)
def test_every_output_cell_has_one_owner(maps, R):
    ms = maps[R]
    assert [m["block"] for m in ms] == list(range(BLOCKS))
    nslots = -(-R // 64)
    units = COLS // 32  # 98 units of 32 columns
    owners = {}
    for m in ms:
        assert m["nslots"] == nslots
        assert 0 <= m["stream"] < STREAMS and 0 <= m["slice"] < SLICES
        slots = list(_slots(m))
        assert all(s < nslots for s in slots)  # no block's row range passes ceil(R / 64)
        for w in range(8):
            c0 = 256 * m["slice"] + 32 * w
            if c0 >= COLS:  # the last slice's idle waves
                assert m["slice"] == SLICES - 1 and w >= 2
                continue
            assert c0 + 32 <= COLS
            for s in slots:
                key = (s, c0 // 32)
                assert key not in owners, (key, owners[key], (m["block"], w))
                owners[key] = (m["block"], w)
    assert len(owners) == nslots * units


def test_streams_sit_on_one_xcd(maps):
    ms = maps[ROWS[-1]]
    # what round-robin dispatch does with the block index
    assert all(m["xcd"] == m["block"] % 8 and m["pos"] == m["block"] // 8 for m in ms)
    assert sorted((m["stream"], m["slice"]) for m in ms) == [(j, s) for j in range(STREAMS) for s in range(SLICES)]
    per_xcd = [sum(1 for m in ms if m["xcd"] == x) for x in range(8)]
    straddlers = 0
    for j in range(STREAMS):
        blk = sorted((m for m in ms if m["stream"] == j), key=lambda m: m["slice"])
        by_xcd = {}
        for m in blk:
            by_xcd.setdefault(m["xcd"], []).append(m["pos"])
        if len(by_xcd) == 1:
            (pos,) = by_xcd.values()
            assert pos == list(range(pos[0], pos[0] + SLICES))  # consecutive, in slice order
            continue
        # a straddling stream: the tail of one XCD's blocks, then the head of the next XCD's
        straddlers += 1
        assert len(by_xcd) == 2
        x0, x1 = sorted(by_xcd)
        assert x1 == x0 + 1
        p0, p1 = by_xcd[x0], by_xcd[x1]
        assert p0 == list(range(p0[0], per_xcd[x0])) and p1 == list(range(0, len(p1)))
    assert straddlers <= 7  # at most one per XCD boundary


def _frag_addrs(g, ks):
    """byte addresses of the kernel's ds_read_b128 of row tile g, k-step ks (one LDS slot)"""
    out = []
    for lane in range(64):
        G, l15 = lane >> 4, lane & 15
        q = ks & 3
        fb_off = l15 * 1024 + ((((q ^ (l15 >> 2)) << 2) | (G ^ (l15 & 3))) << 4)
        out.append(fb_off + g * 16384 + (ks >> 2) * 256)
    return out


def test_b_fragment_reads_are_conflict_free_and_read_the_right_chunks():
    insts = []
    for g in range(4):
        for ks in range(16):
            addrs = _frag_addrs(g, ks)
            insts.append(("b128", addrs))
            for lane, a in enumerate(addrs):
                row, pos = a // 1024, (a % 1024) // 16
                assert row == 16 * g + (lane & 15)
                # the DMA puts source chunk lane ^ (row & 15) at position `lane` of the row
                assert pos ^ (row & 15) == 4 * ks + (lane >> 4)
    c, i = lds.report("fc_dgrad_wreg B fragments", insts)
    assert c == i == 4 * 64
    # unswizzled, the 16 rows of a fragment sit on the same banks
    flat = [("b128", [(lane & 15) * 1024 + (lane >> 4) * 16 for lane in range(64)])]
    assert lds.cycles(flat[0][1], "b128") >= 8 * lds.ideal("b128")
