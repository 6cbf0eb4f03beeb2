"""The half-width FAST arc chunk's min / max network (csrc/fast.hip,
arc_chunk_half), emulated in numpy with the kernel's index algebra, against
the direct definition of the arc strength

    s = max(v - min_k max9_k(ring), max_k min9_k(ring) - v)

(max9_k / min9_k over the 9-arc starting at ring position k).  The kernel
holds the 16 ring values in 8 registers -- position k in register k's low
16-bit half, k + 8 in its high half -- so an index past 7 is the same register
with its halves exchanged (a source-half select of the packed instruction),
and every packed 3-input op yields entries k and k + 8 of its result at once.
Runs on the CPU."""
import numpy as np

# (first, second, third) source index of output register k; an index >= 8 is
# register index - 8 with its halves exchanged
RUN3 = [(0, 1, 2), (1, 2, 3), (2, 3, 4), (3, 4, 5), (4, 5, 6), (5, 6, 7), (6, 7, 8), (7, 8, 9)]
ARC9 = [(0, 3, 6), (1, 4, 7), (2, 5, 8), (3, 6, 9), (4, 7, 10), (5, 8, 11), (6, 9, 12), (7, 10, 13)]
# the reduction over the 8 arc registers: the accumulator A with two more
# registers per step (the last one twice), then A with its own exchanged halves
REDUCE = [(0, 1, 2), ("A", 3, 4), ("A", 5, 6), ("A", 7, 7)]


def _swap(x):
    return (x >> np.uint32(16)) | ((x & np.uint32(0xFFFF)) << np.uint32(16))


def _pk3(op, a, b, c):
    """packed 3-input op on both 16-bit halves of u32 arrays"""
    m = np.uint32(0xFFFF)
    lo = op(op(a & m, b & m), c & m)
    hi = op(op(a >> np.uint32(16), b >> np.uint32(16)), c >> np.uint32(16))
    return lo | (hi << np.uint32(16))


def _src(regs, i):
    return regs[i] if i < 8 else _swap(regs[i - 8])


def _step(op, regs, table):
    return [_pk3(op, _src(regs, a), _src(regs, b), _src(regs, c)) for a, b, c in table]


def _reduce(op, regs):
    acc = None
    for a, b, c in REDUCE:
        acc = _pk3(op, regs[a] if a != "A" else acc, regs[b], regs[c])
    return _pk3(op, acc, _swap(acc), _swap(acc)) & np.uint32(0xFFFF)


def half_network(ring, v):
    """ring (n, 16) u8, v (n,) u8 -> arc strength (n,) int, as arc_chunk_half computes it"""
    r32 = ring.astype(np.uint32)
    regs = [r32[:, k] | (r32[:, k + 8] << np.uint32(16)) for k in range(8)]
    hi9 = _step(np.maximum, _step(np.maximum, regs, RUN3), ARC9)
    lo9 = _step(np.minimum, _step(np.minimum, regs, RUN3), ARC9)
    a = _reduce(np.minimum, hi9).astype(np.int64)  # min over the 16 arcs of the arc's max
    b = _reduce(np.maximum, lo9).astype(np.int64)  # max over the 16 arcs of the arc's min
    vv = v.astype(np.int64)
    return np.maximum(vv - a, b - vv)


def direct(ring, v):
    idx = (np.arange(16)[:, None] + np.arange(9)[None, :]) % 16  # (start, position in arc)
    arcs = ring[:, idx]                                            # (n, 16, 9)
    vv = v.astype(np.int64)
    return np.maximum(vv - arcs.max(axis=2).min(axis=1).astype(np.int64),
                      arcs.min(axis=2).max(axis=1).astype(np.int64) - vv)


def _special_rings():
    rings, vs = [], []
    for val in (0, 1, 127, 128, 254, 255):  # all equal
        for v in (0, val, 255):
            rings.append(np.full(16, val))
            vs.append(v)
    for rot in range(16):  # monotone (from every start), rising and falling
        up = np.roll(np.arange(16) * 17, rot)
        for ring in (up, 255 - up):
            for v in (0, 100, 255):
                rings.append(ring)
                vs.append(v)
    for pos in range(16):  # a single outlier, at every position
        for bg, out in ((100, 0), (100, 255), (0, 255), (255, 0), (30, 29)):
            ring = np.full(16, bg)
            ring[pos] = out
            for v in (bg, out, 0, 255):
                rings.append(ring)
                vs.append(v)
    for pos in range(16):  # an arc of exactly 9 and of exactly 8 bright points, at every position
        for n in (8, 9):
            ring = np.full(16, 10)
            ring[(pos + np.arange(n)) % 16] = 200
            rings.append(ring)
            vs.append(100)
    return np.array(rings, np.uint8), np.array(vs, np.uint8)


def test_index_tables_are_the_circular_runs():
    """RUN3 / ARC9 are (k, k + 1, k + 2) and (k, k + 3, k + 6): three 3-runs
    tile the 9-arc from k; register k's high half is entry k + 8."""
    assert RUN3 == [(k, k + 1, k + 2) for k in range(8)]
    assert ARC9 == [(k, k + 3, k + 6) for k in range(8)]
    for k in range(16):
        runs = [{(k + 3 * j + i) % 16 for i in range(3)} for j in range(3)]
        assert set().union(*runs) == {(k + i) % 16 for i in range(9)}


def test_half_network_random_rings():
    rng = np.random.default_rng(0xFA57)
    ring = rng.integers(0, 256, (100_000, 16), dtype=np.uint8)
    v = rng.integers(0, 256, 100_000, dtype=np.uint8)
    # a second population near the centre value, where arcs of both signs occur
    near = np.clip(v[:, None].astype(np.int64) + rng.integers(-40, 41, (100_000, 16)), 0, 255).astype(np.uint8)
    for r in (ring, near):
        np.testing.assert_array_equal(half_network(r, v), direct(r, v))


def test_half_network_special_rings():
    ring, v = _special_rings()
    np.testing.assert_array_equal(half_network(ring, v), direct(ring, v))
    # the corner test itself: a 9-arc brighter than v + t exists iff s >= t + 1
    s = direct(ring, v)
    arc9 = (ring[-32:].astype(int) == 200)
    assert np.array_equal(s[-32:] > 20, arc9.sum(axis=1) == 9)
