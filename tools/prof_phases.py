#!/usr/bin/env python3
"""Reads the in-kernel phase records written by `tools/colbench_prof --prof DIR` (lbm_kernel_col.hpp, LBM_COL_PROF) and
prints, per kernel variant: the clock calibration, the distribution of every phase over the blocks (load issue -> level 1
done, then one entry per level / step), how many blocks a CU holds at once and how their phases overlap; block lifetimes for three
tile classes (lean, wall, other general: tile_classes), inside wall tiles the level times of the waves the per-wave verdict sends down
the lean path against the others, and per XCD the end of its last block.
A record is ONE whole-domain launch (y_start = 0, y_end = ny): colbench issues no row-range launches and the record is indexed by the
tile index within a launch, so the per-XCD end times of each range kernel of a `split` launch are not reported here
(profiles/boundary_waves/README.md §3 says what that would take).
usage: tools/prof_phases.py DIR [--cu N]"""
import csv, glob, os, sys
import numpy as np

def load(path):
    with open(path) as f:
        head = f.readline().strip()
        rows = list(csv.reader(f))
    cols = rows[0]
    data = np.array([[int(v) for v in r] for r in rows[1:]], dtype=np.uint64)
    launch_us = float(head.split("launch_us=")[1])
    return head, launch_us, cols, data

def tile_classes(head, blocks):
    """Of every block index (the tile index the kernel records): its class and, for a wall tile, which of its waves are plain.
    Classes: "lean" (TileFrame::lean, csrc/lbm_kernels.hpp), "wall" (not lean only because its rings touch a wall row or its band is
    partial: a middle tile column, no solid cell near — the tiles whose plain waves take the lean path, wave_plain), "other" (tile
    columns 0 and last, tiles near the disc). The predicates are those of csrc/lbm_kernels.hpp on the lattice tools/colbench.hip builds:
    one whole-domain launch of the fp64 register kernel, the disc at (0.2 nx, 0.5 ny) with radius 0.05 ny. None where the header names
    no register kernel. Returns ({block: class}, {block: [plain per wave]}, NW)."""
    import re
    m = re.search(r"col R=(\d+) NW=(\d+) D=(\d+) (..) (alt)? *p\d+ (\d+)x(\d+) ", head)
    if not m:
        return None
    R, NW, D = int(m.group(1)), int(m.group(2)), int(m.group(3))
    nx, ny = int(m.group(6)), int(m.group(7))
    HW = D - 1
    OW, OH, H = 64 - 2 * HW, R * NW - 2 * HW, R * NW
    nbx, nby = -(-nx // OW), -(-ny // OH)
    cx, cy, r = int(0.2 * nx), int(0.5 * ny), int(0.05 * ny) + 1
    pitch0 = -(-(16 + nx + 1) // 16) * 16                       # (Lattice<double>: 128-byte sub-rows, twelve ghost rows on each side)
    small = 9 * pitch0 * (ny + 24) * 8 + 4096 < 2 ** 32
    cls, plain = {}, {}
    for b in blocks:
        by, bx = divmod(int(b), nbx)
        X0, Y0 = bx * OW, by * OH
        near = X0 - HW <= cx + r and X0 + OW - 1 + HW >= cx - r and Y0 - HW <= cy + r and Y0 + OH - 1 + HW >= cy - r
        xok = X0 >= HW + 1 and X0 + OW + HW <= nx - 1
        lean = (not near and xok and Y0 >= HW + 1 and Y0 + OH + HW <= ny - 1 and Y0 + OH <= ny and small and by < nby)
        cls[b] = "lean" if lean else ("wall" if (xok and not near and small) else "other")
        if cls[b] == "wall":           # wave_plain, y_start = 0, y_end = ny_glob = ny
            out = []
            for w in range(NW):
                ya = Y0 - HW + w * R
                yb, ryb = ya + R - 1, w * R + R - 1
                top = min(ryb + D, 2 * ryb + 1, H)
                out.append(ya >= 1 and yb <= ny - 2 and yb <= ny + HW - 1 and top <= ny - Y0 + 2 * HW and (ya >= Y0 + OH or min(yb, Y0 + OH - 1) < ny))
            plain[b] = out
    return cls, plain, NW

def describe(path, show_cu=None):
    head, launch_us, cols, d = load(path)
    t = d[:, 5:].astype(np.float64)
    used = (t > 0)
    nmarks = int(used.sum(axis=1).max())
    # marks are s_memrealtime samples: 100 MHz, one counter for the whole chip
    us = (t - t[used].min()) * 0.01
    rates = [100.0]
    t0 = 0.0
    span = us[used].max() - us[used].min()
    print(f"== {head[2:]}\n   {len(d)} wave records, {len(set(d[:,0]))} blocks, marks/wave up to {nmarks}; s_memtime {np.mean(rates):.0f} ticks/us "
          f"(per XCD {min(rates):.0f}..{max(rates):.0f}); first mark -> last mark {span:.1f} us, HIP events {launch_us:.1f} us")
    cyc_per_us = 1.0
    t = us
    w0 = d[:, 1] == 0
    tw = t[w0]
    uw = used[w0]
    # phases of wave 0 of every block
    names = []
    ph = []
    for k in range(1, nmarks):
        ok = uw[:, k] & uw[:, k - 1]
        if ok.sum() == 0: continue
        dur = tw[ok, k] - tw[ok, k - 1]
        ph.append((k, dur))
    print("   phase (mark k-1 -> k) of wave 0, us: median / p10 / p90 / max   [blocks]")
    for k, dur in ph:
        print(f"     {k:3d}: {np.median(dur):7.2f} {np.percentile(dur,10):7.2f} {np.percentile(dur,90):7.2f} {dur.max():7.2f}   [{len(dur)}]")
    # per wave index of a block: when the wave starts (relative to its block's first wave) and how long its level 1 takes
    nwv = int(d[:, 1].max()) + 1
    blocks = sorted(set(d[:, 0].tolist()))
    bix = {b: i for i, b in enumerate(blocks)}
    W0 = np.full((len(blocks), nwv), np.nan); W1 = np.full((len(blocks), nwv), np.nan)
    for r in range(len(d)):
        if used[r, 0] and used[r, 1]:
            W0[bix[d[r, 0]], int(d[r, 1])] = t[r, 0]; W1[bix[d[r, 0]], int(d[r, 1])] = t[r, 1]
    b0 = np.nanmin(W0, axis=1)
    print("   per wave index: start after the block's first wave / its level 1 (mark 0 -> 1), us (medians): "
          + " ".join(f"{np.nanmedian(W0[:, k] - b0):.2f}/{np.nanmedian(W1[:, k] - W0[:, k]):.2f}" for k in range(nwv)))
    print(f"   a block's first wave start -> its last wave's level 1 done: median {np.nanmedian(np.nanmax(W1, axis=1) - b0):.2f} us")
    first = tw[:, 0]
    last = np.array([tw[i, uw[i]].max() for i in range(len(tw))])
    life = last - first
    print(f"   block lifetime us: median {np.median(life):.2f}, p10 {np.percentile(life,10):.2f}, p90 {np.percentile(life,90):.2f}; "
          f"first starts: {np.sort(first)[:3].round(2)}, last start {first.max():.2f}, last end {last.max():.2f}")
    # block lifetime by tile class (first mark of any wave -> last mark of any wave of the block): lean, wall, other general
    tc = tile_classes(head, blocks)
    lean = None
    allfirst = np.where(used, t, np.inf).min(axis=1); alllast = np.where(used, t, -np.inf).max(axis=1)
    if tc is not None:
        cls, plain, _ = tc
        lean = {b: cls[b] == "lean" for b in blocks}
        bl = np.array([bix[b] for b in d[:, 0].tolist()])
        bfirst = np.full(len(blocks), np.inf); blast = np.full(len(blocks), -np.inf)
        np.minimum.at(bfirst, bl, allfirst); np.maximum.at(blast, bl, alllast)
        blife = blast - bfirst
        kind = np.array([cls[b] for b in blocks])
        is_lean = kind == "lean"
        for name, sel in (("lean", is_lean), ("general", ~is_lean), ("wall", kind == "wall"), ("other", kind == "other")):
            if sel.sum():
                v = blife[sel]
                print(f"   {name:7s} blocks: {int(sel.sum()):5d}, lifetime us (all waves): median {np.median(v):.2f}, p10 {np.percentile(v,10):.2f}, "
                      f"p90 {np.percentile(v,90):.2f}")
        if is_lean.sum():
            for name, sel in (("general", ~is_lean), ("wall", kind == "wall"), ("other", kind == "other")):
                if sel.sum():
                    print(f"   {name} / lean median lifetime: {np.median(blife[sel]) / np.median(blife[is_lean]):.3f}")
        # inside wall tiles: the time of every level (mark k-1 -> k) of the waves wave_plain passes against the waves it does not
        rows_wall = np.array([cls[b] == "wall" for b in d[:, 0].tolist()])
        if rows_wall.any():
            wp = np.array([cls[b] == "wall" and plain[b][int(w)] for b, w in zip(d[:, 0].tolist(), d[:, 1].tolist())])
            print(f"   wall tiles: {int((rows_wall & wp).sum())} plain wave records, {int((rows_wall & ~wp).sum())} general; level times us, median (p90), "
                  "plain | general, and the waves of lean tiles beside them:")
            rows_lean = np.array([lean[b] for b in d[:, 0].tolist()])
            for k in range(1, nmarks):
                def stat(sel):
                    ok = sel & used[:, k] & used[:, k - 1]
                    if not ok.any(): return "      -      "
                    v = t[ok, k] - t[ok, k - 1]
                    return f"{np.median(v):6.2f} ({np.percentile(v, 90):6.2f})"
                print(f"     {k:3d}: {stat(rows_wall & wp)} | {stat(rows_wall & ~wp)} | lean {stat(rows_lean)}")
    # per XCD: when its last block ends, relative to the launch's end (the last mark of all)
    xall = d[:, 2] & 0xf
    end = alllast.max(); start = allfirst.min()
    ends = {int(k): float(alllast[xall == k].max()) for k in sorted(set(xall.tolist()))}
    med = float(np.median(list(ends.values())))
    print("   per XCD: last block's end before the launch's end, us: " + " ".join(f"x{k}:{end - v:.2f}" for k, v in ends.items()))
    print(f"   slowest XCD ends {max(ends.values()) - med:.2f} us after the median XCD: {100 * (max(ends.values()) - med) / (end - start):.2f} % of the "
          f"launch ({end - start:.1f} us, first mark to last)")
    if lean is not None:
        print("   general blocks per XCD: " + " ".join(f"x{k}:{len(set(d[(xall == k) & ~np.array([lean[b] for b in d[:, 0].tolist()]), 0].tolist()))}"
                                                       for k in ends))
    # residency per CU
    hw = d[w0, 3]; xcc = d[w0, 2] & 0xf
    cu = ((hw >> 8) & 0xf); sh = (hw >> 12) & 1; se = (hw >> 13) & 0x7
    key = (xcc * 8 + se) * 32 + sh * 16 + cu
    keys = sorted(set(key.tolist()))
    print(f"   distinct CUs seen: {len(keys)}; blocks per CU: min {min((key==k).sum() for k in keys)}, max {max((key==k).sum() for k in keys)}")
    # time-average number of resident blocks per CU, and of blocks in the load phase (mark 0 -> 1)
    res = []; both_load = []; both_comp = []
    for kk in keys:
        idx = np.nonzero(key == kk)[0]
        ev = []
        for i in idx:
            ev.append((first[i], +1)); ev.append((last[i], -1))
        ev.sort()
        area = 0.0; cur = 0; prev = ev[0][0]
        for tt, s in ev:
            area += cur * (tt - prev); prev = tt; cur += s
        res.append(area / (ev[-1][0] - ev[0][0]))
    print(f"   time-averaged resident blocks per CU: mean {np.mean(res):.2f} (min {np.min(res):.2f}, max {np.max(res):.2f})")
    if show_cu is not None:
        kk = keys[show_cu % len(keys)]
        idx = np.nonzero(key == kk)[0]
        idx = idx[np.argsort(first[idx])]
        print(f"   timeline of CU key {kk} (xcc {kk//256}, se {(kk//32)%8}, cu {kk%32}): block: marks in us")
        for i in idx:
            print("     b%-5d " % d[w0][i, 0] + " ".join(f"{v:7.2f}" for v in tw[i, uw[i]]))
    return cyc_per_us

if __name__ == "__main__":
    dirn = sys.argv[1]
    show = int(sys.argv[sys.argv.index("--cu") + 1]) if "--cu" in sys.argv else None
    for p in sorted(glob.glob(os.path.join(dirn, "prof_*.csv"))):
        describe(p, show)
