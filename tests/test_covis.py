"""The covisibility graph as a table in HBM and the covisibility part of
KeyFrame::SetBadFlag on it (include/orbgpu_covis.h, csrc/covis.hip, covis.py),
against the sequential restatement tests/covis_ref.py.

Without a device: the exported symbol (fails without the feature), the struct
layout against ctypes, every ORBGPU_ERR_ARG cause, the stand-alone host program
under the address and undefined-behaviour sanitizers
(tests/cpp/covis_args_main.cpp), and the properties of the restatement (those
pass without the feature).

GPU: every comparison is exact -- the data is integers and copied bytes, there
is no tolerance anywhere.  The table is filled with guard bytes before the rows
are uploaded: below a count every entry equals the restatement's, and from the
count that a row had before the call on every byte is the one that was there.
"""
import ctypes
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import covis_ref as cr

ROOT = Path(__file__).resolve().parent.parent
GUARD = 0x5A


def hub_table():
    """20 keyframes, rows of 16: a hub with 14 spokes (4 of them beyond its first 10), two spokes that name each
    other, a stale connection (15 holds 2, 2 does not hold 15) and a keyframe the hub does not hold (16)"""
    n_kf, stride, hub, far = 20, 16, 0, 19
    spokes = list(range(1, 15))
    conn = {hub: [(k, 10 + k) for k in spokes]}
    conn.update({k: [(hub, 10 + k)] for k in spokes})
    conn[3].append((4, 70))
    conn[4] = [(hub, 14), (3, 70)]
    conn[15] = [(2, 33)]
    conn[16] = [(hub, 5), (far, 6)]
    return n_kf, stride, conn


def random_table(n_kf, density, seed):
    """a symmetric random graph, weights 1..40 with many ties, rows in ascending index; stride = the longest row"""
    rng = np.random.default_rng(seed)
    conn = {k: [] for k in range(n_kf)}
    for a in range(n_kf):
        for b in range(a + 1, n_kf):
            if rng.random() < density:
                w = int(rng.integers(1, 41))
                conn[a].append((b, w))
                conn[b].append((a, w))
    conn = {k: sorted(v) for k, v in conn.items()}
    return n_kf, max(1, max(len(v) for v in conn.values())), conn


# ---- CPU: the restatement --------------------------------------------------------------------------------

def test_ordered_list_and_erasure_in_the_restatement():
    """passes without the feature: it asserts on the restatement"""
    # descending weight, ties in descending map order
    assert cr.best_covisibles([(1, 20), (2, 20), (3, 17), (4, 20), (6, 30)]) == [(6, 30), (4, 20), (2, 20), (1, 20), (3, 17)]
    n_kf, stride, conn = hub_table()
    T = cr.Table(n_kf, stride, conn)
    hub = 0
    assert [k for k, _ in T.ord[hub]] == list(range(14, 0, -1)) and T.covis10(hub) == list(range(14, 4, -1))
    assert cr.erase_keyframes(T, [1]) == [cr.OK]  # beyond the hub's first 10: covis10 stays, the list shrinks
    assert T.covis10(hub) == list(range(14, 4, -1)) and len(T.ord[hub]) == 13 and T.conn[1] == T.ord[1] == []
    assert 1 not in [k for k, _ in T.conn[hub]]
    cr.erase_keyframes(T, [14])  # the hub's first
    assert T.covis10(hub) == list(range(13, 3, -1))
    # the stale connection: 15 names 2, 2 does not hold 15 and keeps its rows
    before = (list(T.conn[2]), list(T.ord[2]))
    cr.erase_keyframes(T, [15])
    assert (T.conn[2], T.ord[2]) == before and T.conn[15] == []
    # two that name each other: the second finds its row without the first
    assert cr.erase_keyframes(T, [3, 20, 4]) == [cr.OK, cr.BAD_JOB, cr.OK]
    assert T.conn[3] == T.conn[4] == [] and all(k not in (3, 4) for k, _ in T.conn[hub])
    # a keyframe with fewer than 10 left is padded with -1
    T = cr.Table(n_kf, stride, conn)
    cr.erase_keyframes(T, list(range(1, 8)))
    assert T.covis10(hub) == list(range(14, 7, -1)) + [-1] * 3
    for size, density in ((70, 0.95), (140, 0.97)):
        n, s, c = random_table(size, density, size)
        assert s > 64 and (size < 130 or s > 128)  # rows that cross one and two waves


class HostGraph:
    """The table as flat guard-filled arrays on the host, written as csrc/covis.hip's erase_kernel writes it --
    the shift that leaves the last entry in place, the rank that writes the entries below the new count only --
    so that what assert_table asks of the bytes past a count is checked without a device."""

    def __init__(self, T):
        g = np.frombuffer(bytes([GUARD] * 4), np.int32)[0]
        self.n_kf, self.stride = T.n_kf, T.stride
        self.h = {name: np.full((T.n_kf, T.stride), g, np.int32) for name in ("conn_kf", "conn_w", "ord_kf", "ord_w")}
        self.h.update(n_conn=np.zeros(T.n_kf, np.int32), n_ord=np.zeros(T.n_kf, np.int32), covis10=np.full((T.n_kf, 10), -1, np.int32))
        for k in range(T.n_kf):
            for rows, cnt, a, b in ((T.conn[k], "n_conn", "conn_kf", "conn_w"), (T.ord[k], "n_ord", "ord_kf", "ord_w")):
                self.h[cnt][k] = len(rows)
                for i, (kf, w) in enumerate(rows):
                    self.h[a][k, i], self.h[b][k, i] = kf, w
            self.h["covis10"][k] = T.covis10(k)

    def download(self):
        return {name: a.copy() for name, a in self.h.items()}

    def erase(self, kfs):
        h, out = self.h, []
        for x in kfs:
            if not 0 <= x < self.n_kf:
                out.append(cr.BAD_JOB)
                continue
            for nb in [int(v) for v in h["conn_kf"][x, :h["n_conn"][x]]]:
                if not 0 <= nb < self.n_kf or nb == x:
                    continue
                n = int(h["n_conn"][nb])
                at = [i for i in range(n) if h["conn_kf"][nb, i] == x]
                if not at:
                    continue
                for a in ("conn_kf", "conn_w"):
                    h[a][nb, at[0]:n - 1] = h[a][nb, at[0] + 1:n].copy()
                n -= 1
                h["n_conn"][nb] = h["n_ord"][nb] = n
                keys = sorted(((int(h["conn_w"][nb, i]), i) for i in range(n)), reverse=True)
                for r, (w, i) in enumerate(keys):
                    h["ord_kf"][nb, r], h["ord_w"][nb, r] = h["conn_kf"][nb, i], w
                best = [int(v) for v in h["ord_kf"][nb, :min(n, 10)]]
                h["covis10"][nb] = best + [-1] * (10 - len(best))
            h["n_conn"][x] = h["n_ord"][x] = 0
            h["covis10"][x] = -1
            out.append(cr.OK)
        return out


def test_bytes_past_the_counts_in_a_host_model_of_the_kernel():
    """passes without the feature: the kernel's writes restated on the host, through the same assert_table as the
    GPU tests.  Two keys taken out of one row leave a left-over between the new and the old count."""
    n_kf, stride, conn = hub_table()
    cases = [(n_kf, stride, conn, kfs) for kfs in ([1], [14], [15], [3, 4], [16, n_kf, -1, 0], [2, 2], list(range(1, 8)), [])]
    for size, density in ((1, 0.0), (2, 1.0), (17, 1.0), (70, 0.95)):
        n, s, c = random_table(size, density, size)
        cases.append((n, s, c, [int(k) for k in np.random.default_rng(size).permutation(n)[:max(1, n // 8)]]))
    for n, s, c, kfs in cases:
        T = cr.Table(n, s, c)
        G = HostGraph(T)
        before = G.download()
        assert G.erase(kfs) == cr.erase_keyframes(T, kfs), kfs
        assert_table(G, before, T, kfs)
    T = cr.Table(n_kf, stride, conn)
    G = HostGraph(T)
    G.erase([3, 4])
    assert G.h["conn_kf"][0, 12:14].tolist() == [14, 14] and G.h["n_conn"][0] == 12  # the left-over of the first shift


# ---- without a GPU: the entry point's host side ----------------------------------------------------------

def test_library_has_the_covisibility_entry_point():
    """fails without the feature: the library has no such symbol"""
    import orbgpu
    assert hasattr(orbgpu.lib(), "orbgpu_covis_erase_keyframes_batch_device")


def test_argument_errors_come_before_the_device():
    """every call here is refused or has nothing to do: one with valid arguments would be launched on a machine
    that has a device, on pointers that are not memory; tests/cpp/covis_args_main.cpp makes those"""
    import covis
    L = covis._lib()
    p = ctypes.c_void_p(256)  # never dereferenced

    def graph(**kw):
        g = covis.CovisGraphStruct()
        g.n_kf, g.conn_stride = 2, 8
        for name, _ in covis.CovisGraphStruct._fields_[2:]:
            setattr(g, name, 256)
        for k, v in kw.items():
            setattr(g, k, v)
        return ctypes.byref(g)

    def erase(n=1, kfs=p, g=None, status=p):
        return L.orbgpu_covis_erase_keyframes_batch_device(n, kfs, g if g is not None else graph(), status, None)

    bad = [dict(n=-1), dict(kfs=None), dict(status=None), dict(g=graph(n_kf=-1)), dict(g=graph(conn_stride=0)),
           dict(g=graph(conn_stride=-1)), dict(g=graph(conn_stride=covis.MAX_STRIDE + 1)), dict(g=graph(n_kf=1 << 29))]
    bad += [dict(g=graph(**{k: None})) for k, _ in covis.CovisGraphStruct._fields_[2:]]
    for kw in bad:
        assert erase(**kw) == -1, kw  # ORBGPU_ERR_ARG, not ORBGPU_ERR_NO_DEVICE
    assert L.orbgpu_covis_erase_keyframes_batch_device(1, p, None, p, None) == -1
    assert L.orbgpu_covis_erase_keyframes_batch_device(0, None, None, None, None) == 0
    assert L.orbgpu_covis_erase_keyframes_batch_device(0, None, graph(), None, None) == 0
    assert L.orbgpu_covis_erase_keyframes_batch_device(0, None, graph(n_ord=None), None, None) == -1


@pytest.fixture(scope="module")
def args_main(tmp_path_factory):
    exe = tmp_path_factory.mktemp("covis_args") / "covis_args_main"
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "--cuda-host-only", "-no-hip-rt", "-O2",
                    "-std=c++17", "-Wall", "-ffp-contract=off", "-fno-fast-math", f"-I{ROOT / 'include'}",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    str(ROOT / "tests" / "cpp" / "covis_args_main.cpp")], check=True, capture_output=True)
    return exe


def test_host_side_of_the_entry_point_is_clean_under_the_sanitizers(args_main):
    """the argument checks, compiled for the host with -fsanitize=address,undefined as a program of its own"""
    r = subprocess.run([str(args_main)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout


def test_struct_layout_equals_the_header(args_main):
    import covis
    r = subprocess.run([str(args_main), "sizes"], capture_output=True, text=True, check=True)
    got = {k: int(v) for k, v in re.findall(r"(\S+) (\d+)", r.stdout)}
    G = covis.CovisGraphStruct
    assert got == {"orbgpu_covis_graph": ctypes.sizeof(G), "graph.conn_stride": G.conn_stride.offset,
                   "graph.n_conn": G.n_conn.offset, "graph.ord_kf": G.ord_kf.offset, "graph.covis10": G.covis10.offset}
    hdr = (ROOT / "include" / "orbgpu_covis.h").read_text()
    for name, v in (("ORBGPU_COVIS_BEST", covis.BEST), ("ORBGPU_COVIS_MAX_STRIDE", covis.MAX_STRIDE)):
        assert int(re.search(rf"#define {name} (\d+)", hdr).group(1)) == v
    for name in ("OK", "BAD_JOB"):
        assert int(re.search(rf"ORBGPU_COVIS_{name} = (\d+)", hdr).group(1)) == getattr(covis, name) == getattr(cr, name)


# ---- GPU ----------------------------------------------------------------------------------------------

def _gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def make_graph(torch, T, covis10=None):
    """the restatement's table T in HBM, every byte past a count a guard byte"""
    import covis
    G = covis.CovisGraph(T.n_kf, T.stride, covis10=covis10)
    for t in G.t.values():
        t.view(-1).view(torch.uint8).fill_(GUARD)
    G.upload(T.conn, T.ord)
    return G


def assert_table(G, before, T, where):
    """the table in HBM against the restatement's: the counts, every entry below them and the best 10; from the
    count that the row had before the call on, the bytes that were there before the call.  An erasure only
    shortens a row: the entries between the two counts are left-overs of the shifts (with two keys taken out of
    one row, the first shift writes the entry that the second leaves behind) and are not compared."""
    h = G.download()
    for k in range(T.n_kf):
        for rows, cnt, a, b in ((T.conn[k], "n_conn", "conn_kf", "conn_w"), (T.ord[k], "n_ord", "ord_kf", "ord_w")):
            n, was = len(rows), int(before[cnt][k])
            assert h[cnt][k] == n <= was, (where, k, cnt)
            assert h[a][k, :n].tolist() == [kf for kf, _ in rows] and h[b][k, :n].tolist() == [w for _, w in rows], (where, k, a)
            assert h[a][k, was:].tobytes() == before[a][k, was:].tobytes() and h[b][k, was:].tobytes() == before[b][k, was:].tobytes(), (where, k, a)
        assert h["covis10"][k].tolist() == T.covis10(k), (where, k)


def run_erase(torch, n_kf, stride, conn, kfs):
    """erase `kfs` in one call on a guard-filled table that holds `conn`; compares the statuses and the table with
    the restatement"""
    import covis
    T = cr.Table(n_kf, stride, conn)
    G = make_graph(torch, T)
    before = G.download()
    status = covis.erase_keyframes(G, kfs)
    torch.cuda.synchronize()
    assert status.cpu().numpy().tolist() == cr.erase_keyframes(T, kfs), kfs
    assert_table(G, before, T, kfs)
    return G


@pytest.mark.gpu
def test_gpu_erase_named_cases():
    """the key present and absent (the stale connection), in the neighbour's first 10 and beyond them, two erased
    keyframes that name each other, an index outside the table between them, a keyframe listed twice, an empty
    list"""
    torch = _gpu()
    n_kf, stride, conn = hub_table()
    for kfs in ([1], [14], [15], [3, 4], [16, n_kf, -1, 0], [2, 2], list(range(1, 8)), []):
        run_erase(torch, n_kf, stride, conn, kfs)


@pytest.mark.gpu
@pytest.mark.parametrize("n_kf,density", [(1, 0.0), (2, 1.0), (17, 1.0), (70, 0.95), (140, 0.97)])
def test_gpu_erase_sizes(n_kf, density):
    """rows of 0, 1, 16 (the waves of the workgroup, once each), more than 64 and more than 128 entries, with many
    equal weights: the search, the shift and the ranking cross one and two waves, and a keyframe with more
    neighbours than the workgroup has waves.  Several erased at once, the last of them again alone"""
    torch = _gpu()
    n, stride, conn = random_table(n_kf, density, n_kf)
    rng = np.random.default_rng(n_kf)
    kfs = [int(k) for k in rng.permutation(n)[:max(1, n // 8)]]
    run_erase(torch, n, stride, conn, kfs)
    run_erase(torch, n, stride, conn, kfs[-1:])


@pytest.mark.gpu
def test_gpu_erase_does_not_depend_on_the_run_and_follows_the_list_order():
    """the same list twice gives the same bytes; two lists that differ in order leave the same rows below the
    counts (an erasure commutes), each equal to its own reference"""
    torch = _gpu()
    n, stride, conn = random_table(40, 0.6, 7)
    a = run_erase(torch, n, stride, conn, [5, 9, 30]).download()
    b = run_erase(torch, n, stride, conn, [5, 9, 30]).download()
    assert all(a[k].tobytes() == b[k].tobytes() for k in a)
    c = run_erase(torch, n, stride, conn, [30, 5, 9])
    T = cr.Table(n, stride, conn)
    cr.erase_keyframes(T, [5, 9, 30])
    assert c.lists() == (T.conn, T.ord)


@pytest.mark.gpu
def test_gpu_gather_reads_the_table_in_place():
    """covis_all pointed at the table, the best 10 kept in the first mirror's own covis array: after an erasure on
    the same stream the LBA gather's outputs equal the gather on host-built lists from the restatement's table"""
    torch = _gpu()
    import covis
    import localba
    import localba_map_ref as lr
    import localba_map_scene as ls
    import test_localba_map as tm
    import track
    sc = ls.SCENES["rich"]()
    nm, n_kf = sc["names"], len(sc["mirror"]["kf_bad"])
    # rows whose ordered lists are the scene's covis_all lists: the weight falls with the position
    conn = {k: sorted((int(c), 100 - i) for i, c in enumerate(lst)) for k, lst in enumerate(sc["ba"]["covis_all"])}
    conn[nm["c"]] = [(nm["a"], 98)]  # c names a: erasing c takes it out of a's list
    T = cr.Table(n_kf, 8, conn)
    assert [k for k, _ in T.ord[nm["a"]]] == list(sc["ba"]["covis_all"][nm["a"]])
    mirror, mirror_ba = track.MapMirror(**sc["mirror"]), localba.MapMirrorBA(**sc["ba"])
    G = make_graph(torch, T, covis10=mirror.t["covis"])
    G.attach(mirror_ba)
    before = G.download()
    B = localba.MapLocalBA(mirror, mirror_ba, [nm["a"]], **tm.BIG)
    tm.guard_fill(torch, B)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    status = covis.erase_keyframes(G, [nm["c"]], stream=stream)
    B.gather(stream)
    stream.synchronize()
    assert status.cpu().numpy().tolist() == cr.erase_keyframes(T, [nm["c"]])
    assert_table(G, before, T, "erase c")
    assert [k for k, _ in T.ord[nm["a"]]] == [nm["b"], nm["cb"]]
    listed = dict(sc["ba"], covis_all=[[k for k, _ in T.ord[i]] for i in range(n_kf)])
    want = lr.gather(sc["mirror"], listed, nm["a"], **tm.BIG)
    assert want.status == lr.OK and want.local_kfs == [nm["a"], nm["b"]]
    B.h = {name: B.host(name) for name in B.t if name not in ("gather_ws", "gather_jobs")}
    tm.assert_job(B, 0, want, "gather after the erasure")
    assert mirror.t["covis"].cpu().numpy().view(np.int32).reshape(n_kf, 10)[nm["a"]].tolist() == T.covis10(nm["a"])
