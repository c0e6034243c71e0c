"""Index-arithmetic model of conv_wgrad_col3x3_kernel (climategan_amd/csrc/conv_wgrad.hip): the staging map (which LDS
bytes every DMA lane of every wave fills for a tile: ring slot, plane, dy buffer) and the fragment-read map (which bytes
every lane's transposing reads take), replayed in the kernel's loop order.  Checked: every byte a tile's MFMAs read holds
the x / dy element the MFMA expects and was written by that tile's own stage or carried from the previous tile (rolling
row ring), and the pieces issued for tile t + 1 while tile t multiplies touch no byte tile t reads.  No GPU.

This is a hand copy of the kernel's index arithmetic: only the TL_* / CW_* constants are read from the source.  It checks
the DESIGN (ring, in-flight slots, dy position permutation, lane maps) and does not follow later edits of the kernel --
whoever changes the kernel's maps changes them here too; the kernel itself is covered by tests/test_gpu_wgrad_spade_tile.py."""
import re
from pathlib import Path

import pytest

SRC = (Path(__file__).resolve().parents[1] / "climategan_amd" / "csrc" / "conv_wgrad.hip").read_text()


def const(name):
    m = re.search(r"\b%s\s*=\s*(\d+)" % name, SRC)
    assert m, name
    return int(m.group(1))


TL_W, TL_H, TL_XP = const("TL_W"), const("TL_H"), const("TL_XP")
RING, NA_MAX = const("CW_RING"), const("CW_NA_MAX")
ROW_BYTES = TL_XP * 128
PLANE_BYTES = RING * ROW_BYTES
DYBUF_BYTES = NA_MAX * TL_H * 1024


def swz(r):
    return ((r & 3) << 1) | ((r >> 2) & 1)


class Model:
    def __init__(self, cin_s, cout_s, n, h, w, splits, cg=0):
        self.cig = cin_s // 16
        self.planes = self.cig // 4
        self.nw = self.cig
        self.cin_s, self.cout_s, self.n, self.h, self.w = cin_s, cout_s, n, h, w
        cot = (cout_s + 15) // 16
        groups = -(-cot // NA_MAX)
        self.NA = -(-cot // groups)
        self.ct0 = min(cg * self.NA, cot - self.NA)      # a ragged last group moves up to end at the last tile
        self.na = self.NA
        self.tw, self.th = w // TL_W, h // TL_H
        self.ntiles = n * self.tw * self.th
        self.splits = splits
        self.dyb = self.planes * PLANE_BYTES
        self.lds_bytes = self.dyb + 2 * DYBUF_BYTES

    def tile(self, t):
        tr, r0 = t % self.th, t // self.th
        return r0 // self.tw, tr * TL_H, (r0 % self.tw) * TL_W      # img, ty0, tx0

    def stage(self, t, b, base, restart):
        """{16-byte LDS chunk address: tag}; tag = ('x', img, iy, ix, ch8) / ('dy', img, oy, ox, co8) / 0 (zero fill)"""
        img, ty0, tx0 = self.tile(t)
        out = {}
        for wave in range(self.nw):
            s_plane, s_row = wave % self.planes, wave // self.planes
            for rr in range(2):
                if rr == 1 and not (restart and s_row < 2):
                    continue
                j = 2 + s_row if rr == 0 else s_row
                slot = (base + j) % RING
                iy = ty0 - 1 + j
                dst = s_plane * PLANE_BYTES + slot * ROW_BYTES
                for i5 in range(5):
                    for lane in range(64):
                        prow, qs = lane >> 3, (lane & 7) ^ swz(lane >> 3)
                        ix = tx0 - 4 + 8 * i5 + prow
                        ok = 0 <= iy < self.h and 0 <= ix < self.w
                        addr = dst + i5 * 1024 + lane * 16
                        assert addr not in out
                        out[addr] = ("x", img, iy, ix, s_plane * 8 + qs) if ok else 0
            dyk = -(-self.NA * TL_H // self.nw)
            for k in range(dyk):
                pid = wave + self.nw * k
                a, ty = pid >> 2, pid & 3
                if a >= self.na:
                    continue
                for lane in range(64):
                    pos = lane >> 1
                    px = (pos & 3) | (((pos >> 4) & 1) << 2) | (((pos >> 2) & 3) << 3)
                    co = (self.ct0 + a) * 16 + (lane & 1) * 8
                    addr = self.dyb + b * DYBUF_BYTES + pid * 1024 + lane * 16
                    assert addr not in out
                    out[addr] = ("dy", img, ty0 + ty, tx0 + px, co // 8) if co < self.cout_s else 0
        return out

    def reads(self, t, buf, base):
        """[(8-byte LDS address, expected tag, 8-byte half)] of every fragment read of tile t"""
        img, ty0, tx0 = self.tile(t)
        out = []
        for wave in range(self.nw):
            c_plane, c_grp = (wave >> 2) % self.planes, wave & 3
            for lane in range(64):
                i, g = lane & 15, lane >> 4
                k = i >> 2
                for ty in range(TL_H):
                    for a in range(self.na):
                        a0 = self.dyb + buf * DYBUF_BYTES + (a * TL_H + ty) * 1024 + (4 * g + k) * 32 + (i & 3) * 8
                        ch = (self.ct0 + a) * 16 + (i & 3) * 4
                        for hi in range(2):
                            want = ("dy", img, ty0 + ty, tx0 + 8 * g + k + 4 * hi, ch // 8) if ch < self.cout_s else 0
                            out.append((a0 + 512 * hi, want, (ch % 8) // 4))
                    for tap in range(9):
                        ky, kx = tap // 3, tap % 3
                        slab = c_plane * PLANE_BYTES + ((base + ty + ky) % RING) * ROW_BYTES
                        q0 = 3 + kx
                        chunk = c_grp * 2 + ((i & 3) >> 1)
                        for hi in range(2):
                            qa = q0 + 8 * g + k + 4 * hi
                            addr = slab + qa * 128 + ((chunk ^ swz(qa & 7)) << 4) + (i & 1) * 8
                            iy, ix = ty0 + ty + ky - 1, tx0 + 8 * g + k + 4 * hi + kx - 1
                            ok = 0 <= iy < self.h and 0 <= ix < self.w
                            want = ("x", img, iy, ix, c_plane * 8 + chunk) if ok else 0
                            out.append((addr, want, i & 1))
        return out

    def run(self):
        """replays every split's loop; returns the number of (tile, read) pairs checked"""
        checked = 0
        covered = []
        for split in range(self.splits):
            lds = {}
            t_begin, t_end = self.ntiles * split // self.splits, self.ntiles * (split + 1) // self.splits
            staged, base = False, 0
            for t in range(t_begin, t_end):
                buf = (t - t_begin) & 1
                if not staged:
                    base = 0
                    lds.update(self.stage(t, buf, 0, True))       # behind a barrier: nobody reads meanwhile
                rd = self.reads(t, buf, base)
                for addr, want, half in rd:
                    assert 0 <= addr and addr + 8 <= self.lds_bytes
                    assert (addr & 8) >> 3 == half
                    assert (addr & ~15) in lds, ("never written", t, addr)
                    assert lds[addr & ~15] == want, (t, addr, lds[addr & ~15], want)
                checked += len(rd)
                staged = False
                if t + 1 < t_end and (t + 1) % self.th != 0:
                    nb = (base + TL_H) % RING
                    nxt = self.stage(t + 1, buf ^ 1, nb, False)   # in flight while tile t is read
                    read_chunks = {a & ~15 for a, _, _ in rd}
                    assert not (read_chunks & set(nxt)), ("slot refilled before its last read", t)
                    lds.update(nxt)
                    staged, base_next = True, nb
                if staged:
                    base = base_next
                covered.append(t)
        assert sorted(covered) == list(range(self.ntiles))
        return checked


@pytest.mark.parametrize("case", [
    # cin_s, cout_s, n, h, w, splits
    (128, 80, 2, 16, 32, 1),      # a column of 4 tiles, two images: ring carried over 3 tile boundaries, not across images
    (128, 80, 2, 8, 32, 3),       # ranges that begin in the middle of a column
    (128, 40, 1, 12, 64, 1),      # two columns of three tiles, interior horizontal halo
    (64, 80, 1, 16, 32, 2),       # one plane, four waves
    (128, 136, 1, 8, 32, 1),      # padded channel tail
    (128, 8, 2, 4, 32, 2),        # single tile per image
])
def test_staging_and_fragment_maps(case):
    cin_s, cout_s, n, h, w, splits = case
    cot = (cout_s + 15) // 16
    for cg in range(-(-cot // NA_MAX)):
        m = Model(cin_s, cout_s, n, h, w, splits, cg)
        assert m.lds_bytes <= 160 * 1024
        assert m.run() > 0


def test_lds_budget_matches_the_kernel():
    assert re.search(r"CW_ROW_BYTES = TL_XP \* 128;", SRC)
    assert re.search(r"CW_PLANE_BYTES = CW_RING \* CW_ROW_BYTES;", SRC)
    assert re.search(r"CW_DYBUF_BYTES = CW_NA_MAX \* TL_H \* 1024;", SRC)
    assert 2 * PLANE_BYTES + 2 * DYBUF_BYTES == 140 * 1024
