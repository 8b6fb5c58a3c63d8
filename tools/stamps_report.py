"""Phase shares of the join stream kernel from a saved DG_STAMPS buffer (tools/prof_c5.py
with C5_STAMPS=<file.npy>).  Stamps (s_memrealtime, 100 MHz, lane 0 of each tile):
0 iteration start (a workgroup's first tile: the workgroup's entry), 1 iteration start, 2 tile committed to LDS, 7 next tile's loads issued, 3 merge done, 4 block scan + compaction
list (+ change events) done, 5 previous stripe's counts summed, 6 previous tile written.  Only shares
are meaningful (the stamps add barriers)."""
import sys

import numpy as np


def main(path):
    st = np.load(path).reshape(65536, 16).astype(np.int64)
    ntiles = int(np.nonzero(st[:, 0])[0].max()) + 1
    st = st[:ntiles]
    t0 = st[:, 0].min()
    names = ["commit", "issue", "merge", "scan", "sums", "write"]
    st[st[:, 5] == 0, 5] = st[st[:, 5] == 0, 4]  # first iteration: no previous tile
    d = np.diff(st[:, [1, 2, 7, 3, 4, 5, 6]], axis=1) * 10 / 1000.0
    print(f"tiles={ntiles} span={(st[:, 6].max() - t0) * 10 / 1000:.1f} us")
    for i, nm in enumerate(names):
        print(f"{nm:11s} median {np.median(d[:, i]):6.2f} us  p90 {np.percentile(d[:, i], 90):6.2f}"
              f"  mean {d[:, i].mean():6.2f}")
    it = np.diff(np.sort(st[:, 1]))
    print("per-tile total median", np.median((st[:, 6] - st[:, 1]) * 10 / 1000))
    first = st[:, 8] > 0  # a workgroup's first tile: slot 0 is its entry, 8 and 9 prologue stamps
    if first.any():
        pro = (st[first, 1] - st[first, 0]) * 10 / 1000
        ent = (st[first, 0] - st[first, 0].min()) * 10 / 1000
        for a, b, nm in ((0, 8, "split search"), (8, 9, "first tile issued"), (9, 1, "VV tables + tile landed")):
            x = (st[first, b] - st[first, a]) * 10 / 1000
            print(f"  prologue {nm:24s} median {np.median(x):5.2f} us  p90 {np.percentile(x, 90):5.2f}")
        print(f"prologue (entry -> first iteration) median {np.median(pro):.2f} us  p90 "
              f"{np.percentile(pro, 90):.2f}; entries spread over {ent.max():.2f} us; "
              f"last write {(st[:, 6].max() - st[first, 0].min()) * 10 / 1000:.1f} us after the first entry")
    first = (st[:, 1] - t0) * 10 / 1000  # iteration starts relative to the earliest one
    print("iteration start (us) at deciles:", np.percentile(first, np.arange(0, 101, 10)).round(1))
    print(f"last write done at {(st[:, 6].max() - t0) * 10 / 1000:.1f} us after the first iteration start")
    placement(st, t0)


def placement(st, t0):
    """Which workgroups share a CU (slots 10 and 11 of a workgroup's first tile: XCC_ID and
    HW_ID, 1 + blockIdx), each workgroup's pace, and the pace against the phase offset to
    the CU-mate.  Tiles are walked by stripe position: position x merges tiles x + k*G."""
    G = int((st[:, 11] > 0).sum())
    if G == 0:
        return
    ntiles = len(st)
    hw = st[:G, 10]
    blk = st[:G, 11] - 1
    xcc, se, sh, cu = (hw >> 32) & 15, (hw >> 13) & 7, (hw >> 12) & 1, (hw >> 8) & 15
    key = ((xcc * 8 + se) * 2 + sh) * 16 + cu
    us = lambda v: v * 10 / 1000.0
    # pace: from the first iteration start to the last write, per iteration
    nit = np.array([len(range(x, ntiles, G)) for x in range(G)])
    last = np.array([x + (nit[x] - 1) * G for x in range(G)])
    pace = us(st[last, 6] - st[:G, 1]) / nit
    print(f"placement: G={G} positions on {len(np.unique(key))} CUs, {len(np.unique(xcc))} XCCs; "
          f"position == blockIdx for {(blk == np.arange(G)).mean() * 100:.0f} % of workgroups")
    print("pace (us per iteration) at deciles:", np.percentile(pace, np.arange(0, 101, 10)).round(2))
    # CU-mates, as differences of blockIdx
    mate = np.full(G, -1)
    sizes = {}
    for k in np.unique(key):
        m = np.nonzero(key == k)[0]
        sizes[len(m)] = sizes.get(len(m), 0) + 1
        if len(m) == 2:
            mate[m[0]], mate[m[1]] = m[1], m[0]
    print("workgroups per CU -> CUs:", dict(sorted(sizes.items())))
    pairs = np.nonzero((mate >= 0) & (np.arange(G) < mate))[0]
    if len(pairs):
        dif, cnt = np.unique(np.abs(blk[mate[pairs]] - blk[pairs]), return_counts=True)
        top = np.argsort(-cnt)[:4]
        print("CU-mates' blockIdx differ by:", ", ".join(
            f"{dif[i]} ({cnt[i] * 100.0 / len(pairs):.0f} % of pairs)" for i in top))
        GE = (G + 1) // 2
        opp = ((pairs < GE) != (mate[pairs] < GE)).mean() * 100
        print(f"CU-mates in opposite halves of the stripe (positions < {GE} against the rest): {opp:.0f} % of pairs")
    # pace against the phase offset to the CU-mate: the mean over the common iterations of
    # |start - mate's start| folded into [0, 1/2] of the pair's mean pace
    has = np.nonzero(mate >= 0)[0]
    if len(has):
        off = np.zeros(len(has))
        for i, x in enumerate(has):
            n = min(nit[x], nit[mate[x]])
            a = st[x + np.arange(n) * G, 1]
            b = st[mate[x] + np.arange(n) * G, 1]
            p = (pace[x] + pace[mate[x]]) / 2
            f = (us(np.abs(a - b)) / p) % 1.0
            off[i] = np.minimum(f, 1 - f).mean()
        print("pace by phase offset to the CU-mate (fraction of an iteration, folded to 0..0.5):")
        for lo, hi in ((0, 0.125), (0.125, 0.25), (0.25, 0.375), (0.375, 0.5001)):
            m = (off >= lo) & (off < hi)
            if m.any():
                print(f"  offset {lo:.3f}-{min(hi, 0.5):.3f}: {m.sum():4d} workgroups, pace median "
                      f"{np.median(pace[has][m]):.2f} mean {pace[has][m].mean():.2f} us")
        if len(has) > 2 and off.std() > 0 and pace[has].std() > 0:
            print(f"  correlation of pace with offset: {np.corrcoef(off, pace[has])[0, 1]:+.2f}")
    print("pace by XCC (median us):", " ".join(
        f"{x}:{np.median(pace[xcc == x]):.2f}" for x in np.unique(xcc)))
    q = np.minimum(np.arange(G) * 4 // G, 3)
    print("pace by quarter of the stripe (median us):", " ".join(
        f"{np.median(pace[q == i]):.2f}" for i in range(4) if (q == i).any()))
    if G > 2 and pace.std() > 0:
        print(f"  correlation of pace with position: {np.corrcoef(np.arange(G), pace)[0, 1]:+.2f}")
    # iteration starts per half of the stripe (the classes E and L of the stagger)
    GE = (G + 1) // 2
    ns = int(nit.max())
    print("iteration start per stripe, median us (low half | high half | high - low):")
    for k in range(min(ns, 8)):
        t = np.arange(k * G, min((k + 1) * G, ntiles))
        s = us(st[t, 1] - t0)
        e, l = s[(t - k * G) < GE], s[(t - k * G) >= GE]
        if len(e) and len(l):
            print(f"  stripe {k}: {np.median(e):6.2f} | {np.median(l):6.2f} | {np.median(l) - np.median(e):+5.2f}")


if __name__ == "__main__":
    main(sys.argv[1])
