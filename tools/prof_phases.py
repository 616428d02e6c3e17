#!/usr/bin/env python3
"""Reads the in-kernel phase records written by `tools/colbench_prof --prof DIR` (lbm_kernel_col.hpp, LBM_COL_PROF) and
prints, per kernel variant: the clock calibration, the distribution of every phase over the blocks (load issue -> level 1
done, then one entry per level / step), how many blocks a CU holds at once and how their phases overlap.
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
    """Of every block index (the tile index the kernel records): True where the tile takes the lean path. The predicate is
    TileFrame::lean (csrc/lbm_kernels.hpp) on the lattice tools/colbench.hip builds: one whole-domain launch of the fp64 register kernel,
    the disc at (0.2 nx, 0.5 ny) with radius 0.05 ny. None where the header names no register kernel."""
    import re
    m = re.search(r"col R=(\d+) NW=(\d+) D=(\d+) (..) (alt)? *p\d+ (\d+)x(\d+) ", head)
    if not m:
        return None
    R, NW, D = int(m.group(1)), int(m.group(2)), int(m.group(3))
    nx, ny = int(m.group(6)), int(m.group(7))
    HW = D - 1
    OW, OH = 64 - 2 * HW, R * NW - 2 * HW
    nbx, nby = -(-nx // OW), -(-ny // OH)
    cx, cy, r = int(0.2 * nx), int(0.5 * ny), int(0.05 * ny) + 1
    pitch0 = -(-(16 + nx + 1) // 16) * 16                       # (Lattice<double>: 128-byte sub-rows, twelve ghost rows on each side)
    small = 9 * pitch0 * (ny + 24) * 8 + 4096 < 2 ** 32
    out = {}
    for b in blocks:
        by, bx = divmod(int(b), nbx)
        X0, Y0 = bx * OW, by * OH
        near = X0 - HW <= cx + r and X0 + OW - 1 + HW >= cx - r and Y0 - HW <= cy + r and Y0 + OH - 1 + HW >= cy - r
        out[b] = (not near and X0 >= HW + 1 and X0 + OW + HW <= nx - 1 and Y0 >= HW + 1 and Y0 + OH + HW <= ny - 1
                  and Y0 + OH <= ny and small and by < nby)
    return out

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
    # block lifetime by tile class (first mark of wave 0 -> last mark of any wave of the block), lean against general
    lean = tile_classes(head, blocks)
    allfirst = np.where(used, t, np.inf).min(axis=1); alllast = np.where(used, t, -np.inf).max(axis=1)
    if lean is not None:
        bl = np.array([bix[b] for b in d[:, 0].tolist()])
        bfirst = np.full(len(blocks), np.inf); blast = np.full(len(blocks), -np.inf)
        np.minimum.at(bfirst, bl, allfirst); np.maximum.at(blast, bl, alllast)
        blife = blast - bfirst
        is_lean = np.array([lean[b] for b in blocks])
        for name, sel in (("lean", is_lean), ("general", ~is_lean)):
            if sel.sum():
                v = blife[sel]
                print(f"   {name:7s} blocks: {int(sel.sum()):5d}, lifetime us (all waves): median {np.median(v):.2f}, p10 {np.percentile(v,10):.2f}, "
                      f"p90 {np.percentile(v,90):.2f}")
        if is_lean.sum() and (~is_lean).sum():
            print(f"   general / lean median lifetime: {np.median(blife[~is_lean]) / np.median(blife[is_lean]):.3f}")
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
