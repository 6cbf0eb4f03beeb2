"""DistributeOctTree (ORBextractor.cpp:541-770) restated as the level-synchronous
passes of csrc/octree.hip, in plain Python (TESTS ONLY).

Two forms of the first main passes, which must agree:
  * pass by pass: every node with > 1 key is divided from its own keys;
  * fused: every key's path through three subdivisions below its root is
    counted once, the passes are replayed on the counts alone, and the keys
    get their nodes from one table -- what the kernel does by default.
`distribute` returns the output keys in list order and, for the fused form,
how many passes the replay took and whether it ended at the switch to the
finishing loop, so that a test can tell which branch a level takes.
"""
from __future__ import annotations

import numpy as np

EDGE = 19
BORDER = EDGE - 3
f32 = np.float32


def level_geometry(width, height, nlevels=8, scale_factor=1.2):
    """(w, h) of every pyramid level (ORBextractor::ComputePyramid)."""
    out, s = [], f32(1.0)
    for l in range(nlevels):
        inv = f32(1.0) / s
        out.append((int(np.rint(f32(width) * inv)), int(np.rint(f32(height) * inv))))
        s = f32(s * f32(scale_factor))
    return out


def _mid(a, b):
    return a + ((b - a + 1) >> 1)  # ceil((float)(UR.x - UL.x) / 2), ExtractorNode::DivideNode


def _quad(box, x, y):
    x0, y0, x1, y1 = box
    return (0 if x < _mid(x0, x1) else 1) + (0 if y < _mid(y0, y1) else 2)


def _child(box, q):
    x0, y0, x1, y1 = box
    mx, my = _mid(x0, x1), _mid(y0, y1)
    return (mx if q & 1 else x0, my if q & 2 else y0, x1 if q & 1 else mx, y1 if q & 2 else my)


class _Node:
    __slots__ = ("box", "keys", "cnt", "seq", "gid", "depth")

    def __init__(self, box, keys, seq, cnt=None, gid=0, depth=0):
        self.box, self.keys, self.seq = box, keys, seq
        self.cnt = len(keys) if cnt is None else cnt
        self.gid, self.depth = gid, depth


def _roots(xys, w, h):
    bw, bh = (w - EDGE + 3) - BORDER, (h - EDGE + 3) - BORDER
    nini = int(np.round(f32(bw) / f32(bh)))
    hx = f32(bw) / f32(nini)
    buckets = [[] for _ in range(nini)]
    for k, (x, _, _) in enumerate(xys):
        buckets[min(int(f32(x) / hx), nini - 1)].append(k)
    nodes = [_Node((int(hx * f32(r)), 0, int(hx * f32(r + 1)), bh), b, r) for r, b in enumerate(buckets) if b]
    return nodes, nini


def _push(nodes, flagged, child_counts, nseq, child_of):
    """The next list: children of the flagged nodes (in the given division order)
    in reverse push order, then the other nodes in their old order."""
    pushed = []
    for i in flagged:
        for q in range(4):
            if child_counts[i][q] > 0:
                pushed.append(child_of(nodes[i], q, nseq + len(pushed)))
    fl = set(flagged)
    return pushed[::-1] + [n for i, n in enumerate(nodes) if i not in fl], len(pushed)


def _split_by_keys(xys):
    def counts(n):
        c = [0, 0, 0, 0]
        for k in n.keys:
            c[_quad(n.box, xys[k][0], xys[k][1])] += 1
        return c

    def child(n, q, seq):
        return _Node(_child(n.box, q), [k for k in n.keys if _quad(n.box, xys[k][0], xys[k][1]) == q], seq)

    return counts, child


def _pass(nodes, N, nseq, inner, counts, child):
    """One pass; returns (next list, children pushed, children with > 1 key)."""
    cc = [counts(n) if n.cnt > 1 else [0, 0, 0, 0] for n in nodes]
    div = [i for i, n in enumerate(nodes) if n.cnt > 1]
    if inner:
        div.sort(key=lambda i: (nodes[i].cnt, nodes[i].seq), reverse=True)
        size, flagged = len(nodes), []
        for i in div:
            flagged.append(i)
            size += sum(c > 0 for c in cc[i]) - 1
            if size >= N:
                break
    else:
        flagged = div
    new, C = _push(nodes, flagged, cc, nseq, child)
    nexp = sum(c > 1 for i in flagged for c in cc[i])
    return new, C, nexp


def distribute(cands, w, h, N, fused=True):
    """cands: (n, 3) int (x, y, response) in candidate order, level size (w, h).
    Returns (output keys (m, 3), info) with info = dict(fused form taken, fused passes, inner at
    the hand-over, the list sizes after each pass, the empty children dropped by each
    fused pass)."""
    xys = [tuple(int(v) for v in r) for r in cands]
    nodes, nini = _roots(xys, w, h)
    nseq, inner, sizes, replayed, max_root_keys = nini, False, [], 0, max([n.cnt for n in nodes], default=0)
    counts, child = _split_by_keys(xys)
    done, dropped = not nodes, []
    fused = fused and 1 <= len(nodes) <= 4  # (more roots: the level goes pass by pass)
    if fused:
        # one sweep: bins[root * 64 + q1 * 16 + q2 * 4 + q3]
        bins = [0] * (64 * len(nodes))
        key_bin = []
        root_of = {}
        for r, n in enumerate(nodes):
            n.gid, n.depth = r, 0
            for k in n.keys:
                root_of[k] = r
        for k, (x, y, _) in enumerate(xys):
            r = root_of[k]
            box, b = nodes[r].box, r
            for _ in range(3):
                q = _quad(box, x, y)
                box, b = _child(box, q), b * 4 + q
            key_bin.append(b)
            bins[b] += 1

        def count_of(gid, depth):
            sh = 2 * (3 - depth)
            return sum(bins[gid << sh:(gid + 1) << sh])

        for p in (1, 2, 3):
            if len(nodes) > 64:
                break
            assert all(n.depth == p - 1 for n in nodes if n.cnt > 1)
            empty = sum(count_of(n.gid * 4 + q, n.depth + 1) == 0 for n in nodes if n.cnt > 1 for q in range(4))
            new, C, nexp = _pass(nodes, N, nseq, False,
                                 lambda n: [count_of(n.gid * 4 + q, n.depth + 1) for q in range(4)],
                                 lambda n, q, seq: _Node(_child(n.box, q), [], seq, count_of(n.gid * 4 + q, n.depth + 1),
                                                         n.gid * 4 + q, n.depth + 1))
            if len(new) >= N or len(new) == len(nodes):
                break  # the pass that ends the distribution is the general code's
            nodes, nseq, replayed = new, nseq + C, p
            dropped.append(empty)
            sizes.append(len(nodes))
            if len(nodes) + 3 * nexp > N:
                inner = True
                break
        table = {}
        for i, n in enumerate(nodes):
            sh = 2 * (3 - n.depth)
            for b in range(n.gid << sh, (n.gid + 1) << sh):
                table[b] = i
            n.keys = []
        for k, b in enumerate(key_bin):
            nodes[table[b]].keys.append(k)
        assert all(n.cnt == len(n.keys) for n in nodes)
    inner_at_handover = inner
    while not done:
        new, C, nexp = _pass(nodes, N, nseq, inner, counts, child)
        done = len(new) >= N or len(new) == len(nodes)
        if not inner and len(new) + 3 * nexp > N:
            inner = True
        nodes, nseq = new, nseq + C
        sizes.append(len(nodes))
    out = []
    for n in nodes:
        best = n.keys[0]
        for k in n.keys:
            if xys[k][2] > xys[best][2]:
                best = k
        out.append(xys[best])
    info = dict(fused=fused, replayed=replayed, inner=inner_at_handover, sizes=sizes, roots=nini, max_root_keys=max_root_keys,
                dropped=dropped)
    return np.asarray(out, np.int32).reshape(-1, 3), info
