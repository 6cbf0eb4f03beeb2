"""The keyframe database on the device (include/orbgpu_kfdb.h, csrc/kfdb.hip,
kfdb.py) against oracle/kfdb_ref.py called sequentially in batch order
(tests/kfdb_scene.py).

Without a device: the exported symbols (fails without the feature), the
stand-alone host program under the address and undefined-behaviour sanitizers
(tests/cpp/kfdb_args_main.cpp), the struct layouts, argument errors through
the library, and three properties of the restatement.

GPU: every integer of the result, every candidate row, the bits of every float
and the final mRelocScore array equal to the reference: the size sweep with
and without loop queries, hand-built edge scenes, list order, batch semantics,
CAPACITY and every BAD_JOB cause, KL within one float ulp, and the chain
ComputeBoW -> detect -> emit -> SearchByBoW -> PnPsolver set-up -> one pass of
the loop on one stream against a RelocBurst built on the host.
"""
import ctypes
import functools
import os
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import kfdb_scene as ks

ROOT = Path(__file__).resolve().parent.parent
f32 = np.float32
RELOC, LOOP = ks.RELOC, ks.LOOP
GUARD = 0x5A5A5A5A


def bits(x):
    return np.asarray(x, f32).view(np.uint32)


# ---- scenes ---------------------------------------------------------------------------

def tiny(bows, covis=None, in_db=None, reloc0=None, scoring=0):
    """a hand-built database: bows per keyframe, covis per keyframe (lists)"""
    n = len(bows)
    covis = covis or {}
    kfs = [{"bow": dict(b), "connected": set(), "best_covis": list(covis.get(k, []))} for k, b in enumerate(bows)]
    return {"scoring": scoring, "n_words": 64, "kfs": kfs, "in_db": list(range(n)) if in_db is None else list(in_db),
            "kf_bad": np.zeros(n, np.uint8),
            "reloc0": np.linspace(0.3, 0.9, n).astype(f32) if reloc0 is None else np.asarray(reloc0, f32)}


def words(ws, v):
    return {w: v for w in ws}


QUERY10 = {"kind": RELOC, "bow": words(range(10), 0.1)}  # with L1, a keyframe scores the sum of min(0.1, its value)


@functools.lru_cache(maxsize=None)
def order_scenes():
    lo, hi = range(0, 5), range(5, 10)
    return {
        # the higher index shares an earlier query word: list order 1, 0
        "first_word": (tiny([words(hi, 0.2), words(lo, 0.2)]), [QUERY10]),
        # the same first word, add() order 1 then 0
        "add_rank": (tiny([words(lo, 0.2), words(lo, 0.2)], in_db=[1, 0]), [QUERY10]),
        # entries 0 and 1 both name keyframe 2 as pBestKF, entry 3 names 4: [2, 4], each once
        "same_best": (tiny([words(lo, 0.05), words(lo, 0.05), words(lo, 0.1), words(hi, 0.07), words(hi, 0.1)],
                           covis={0: [2], 1: [2], 3: [4]}), [QUERY10]),
        # LOOP: keyframe 1 scores 0.25 < minScore 0.3 and still adds to keyframe 0's accScore
        "below_min": (tiny([words(lo, 0.1), words(lo, 0.05)], covis={0: [1]}),
                      [{"kind": LOOP, "bow": words(range(10), 0.1), "connected": [], "covisible": None, "min_score": 0.3}]),
        # keyframe 1 shares one word: listed, not scored, read stale by entry 0; the second query scores it
        "stale": (tiny([words(lo, 0.1), words([0], 0.02)], covis={0: [1]}, reloc0=[0.0, 0.7]),
                  [QUERY10, {"kind": RELOC, "bow": words([0], 0.1)}, QUERY10]),
    }


@functools.lru_cache(maxsize=None)
def sweep(scoring, n_kf):
    """the base scene with two loop queries among the six relocalisation queries; the loop queries' keyframes
    are not in the database yet (LoopClosing::DetectLoop), except in the scene of one keyframe"""
    sc, rq = ks.base(scoring, n_kf)
    a, b = n_kf - 1, n_kf // 2
    if n_kf > 1:
        sc["in_db"] = [k for k in range(n_kf) if k not in (a, b)]
    queries = [rq[0], rq[1], ks.loop_query(sc, a), rq[2], rq[3], ks.loop_query(sc, b, covisible=False, min_score=0.05),
               rq[4], rq[5]]
    want, final = ks.reference(sc, queries)
    return sc, queries, want, final


@functools.lru_cache(maxsize=None)
def edge_scene():
    """the base scene of 65 keyframes (scoring 0) with the hand-built additions"""
    sc, rq = ks.base(0, 65)
    used = set().union(*[set(q["bow"]) for q in rq])
    free = [w for w in range(sc["n_words"]) if w not in used]
    kfs = sc["kfs"]
    kfs.append({"bow": {}, "connected": set(), "best_covis": [3, 64]})                      # 65: an empty BowVector
    kfs.append({"bow": words(free[:2], 0.5), "connected": set(), "best_covis": []})          # 66, 67: words no
    kfs.append({"bow": words(free[2:5], 0.3), "connected": set(), "best_covis": [66]})       # relocalisation query has
    n = len(kfs)
    sc["in_db"] = [k for k in range(n) if k not in (10, 11, 64)]  # 10, 11 erased (still in covis rows), 64 not added yet
    sc["kf_bad"] = np.zeros(n, np.uint8)
    sc["kf_bad"][60] = 1
    sc["reloc0"] = np.linspace(-0.25, 1.25, n).astype(f32)
    first = rq[0]["bow"]
    cut = lambda m: {"kind": RELOC, "bow": {w: first[w] for w in sorted(first)[:m]}}  # noqa: E731
    lq = ks.loop_query(sc, 64)
    lq["covisible"] = lq["covisible"] + [10, 60]  # an erased covisible is scored, a bad one is skipped
    self_query = {"kind": LOOP, "bow": dict(kfs[30]["bow"]), "connected": [], "covisible": None, "min_score": 0.0}
    queries = [rq[0], cut(0), cut(1), lq, cut(64), cut(65), rq[3], self_query, rq[1]]
    want, final = ks.reference(sc, queries)
    return sc, queries, want, final


# ---- CPU ---------------------------------------------------------------------------------

def test_library_exports_the_keyframe_database():
    """fails without the feature"""
    import orbgpu
    L = orbgpu.lib()
    for name in ("orbgpu_kfdb_detect_workspace_bytes", "orbgpu_kfdb_detect_batch_device",
                 "orbgpu_kfdb_emit_reloc_batch_device"):
        assert hasattr(L, name), name
    import kfdb
    import reloc
    assert hasattr(reloc.RelocBurst, "from_tables") and kfdb.MAX_KEYFRAMES >= 8192


def test_argument_errors_come_before_the_device():
    import kfdb
    L = kfdb._lib()
    D = kfdb.KfdbStruct(n_kf=10, scoring=0, n_bow_total=100)
    p = ctypes.addressof(ctypes.create_string_buffer(256))
    d = ctypes.addressof(D)
    assert L.orbgpu_kfdb_detect_batch_device(-1, p, d, 4, p, p, p, None, None, None) == -1
    assert L.orbgpu_kfdb_detect_batch_device(1, p, d, 0, p, p, p, None, None, None) == -1
    assert L.orbgpu_kfdb_detect_batch_device(1, p, None, 4, p, p, p, None, None, None) == -1
    assert L.orbgpu_kfdb_detect_batch_device(1, p, d, 4, p, None, p, None, None, None) == -1
    assert L.orbgpu_kfdb_detect_batch_device(1, p, d, 4, p, p, None, None, None, None) == -1
    big = kfdb.KfdbStruct(n_kf=kfdb.MAX_KEYFRAMES + 1, scoring=0, n_bow_total=100)
    assert L.orbgpu_kfdb_detect_batch_device(1, p, ctypes.addressof(big), 4, p, p, p, None, None, None) == -1
    assert L.orbgpu_kfdb_detect_batch_device(0, None, d, 4, None, p, p, None, None, None) == 0
    assert L.orbgpu_kfdb_emit_reloc_batch_device(1, p, p, p, 65, None, p, p, p, p, p, p, None) == -1
    assert L.orbgpu_kfdb_emit_reloc_batch_device(0, None, None, None, 8, None, None, None, None, None, None, None,
                                                 None) == 0
    assert L.orbgpu_kfdb_detect_workspace_bytes(64, 2000) > 0


@pytest.fixture(scope="module")
def kfdb_args_main(tmp_path_factory):
    exe = tmp_path_factory.mktemp("kfdb_args") / "kfdb_args_main"
    subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-x", "hip", "--cuda-host-only", "-no-hip-rt", "-O2",
                    "-std=c++17", "-Wall", "-ffp-contract=off", "-fno-fast-math", f"-I{ROOT / 'include'}",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-o", str(exe),
                    str(ROOT / "tests" / "cpp" / "kfdb_args_main.cpp")], check=True, capture_output=True)
    return exe


def test_host_side_of_the_entry_points_is_clean_under_the_sanitizers(kfdb_args_main):
    """every argument error before the device, n == 0 and the carving of the opaque block from a null base,
    compiled for the host with -fsanitize=address,undefined as a program of its own"""
    r = subprocess.run([str(kfdb_args_main)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout


def test_struct_layouts_equal_the_header(kfdb_args_main):
    import kfdb
    r = subprocess.run([str(kfdb_args_main), "sizes"], capture_output=True, text=True, check=True)
    got = dict(re.findall(r"(\S+) (\d+)", r.stdout))
    D, Q, R = kfdb.KfdbStruct, kfdb.KfdbQuery, kfdb.KfdbResult
    want = {"orbgpu_kfdb": ctypes.sizeof(D), "orbgpu_kfdb_query": ctypes.sizeof(Q), "orbgpu_kfdb_result": ctypes.sizeof(R),
            "db.n_bow_total": D.n_bow_total.offset, "db.in_db": D.in_db.offset, "db.kf_bad": D.kf_bad.offset,
            "db.bow_values": D.bow_values.offset, "db.reloc_score": D.reloc_score.offset,
            "query.n_covisible": Q.n_covisible.offset, "query.min_score": Q.min_score.offset,
            "query.words": Q.words.offset, "query.d_n_words": Q.d_n_words.offset, "query.covisible": Q.covisible.offset,
            "result.n_candidates": R.n_candidates.offset, "result.min_score": R.min_score.offset,
            "result.best_acc_score": R.best_acc_score.offset, "max_keyframes": kfdb.MAX_KEYFRAMES,
            "max_words": kfdb.MAX_WORDS}
    assert {k: int(v) for k, v in got.items()} == want


def test_list_order_is_first_shared_word_then_add_order():
    """passes without the feature: it asserts on the restatement"""
    sc = order_scenes()
    for name, cands in (("first_word", [1, 0]), ("add_rank", [1, 0]), ("same_best", [2, 4])):
        want, _ = ks.reference(*sc[name])
        assert want[0]["candidates"] == cands, name
    assert [k for _, k in ks.reference(*sc["same_best"])[0][0]["acc_list"]] == [2, 2, 2, 4, 4]


def test_stale_reloc_score_is_read_and_depends_on_the_queries_before():
    """passes without the feature: it asserts on the restatement"""
    scene, queries = order_scenes()["stale"]
    want, final = ks.reference(scene, queries)
    assert [w["stale"] for w in want] == [1, 0, 1]
    assert want[0]["acc_list"] == [(f32(f32(0.5) + f32(0.7)), 1)]  # what the array held at the call: keyframe 1 wins
    assert want[2]["acc_list"] == [(f32(f32(0.5) + f32(0.02)), 0)]  # what the second query wrote
    assert want[0]["candidates"] == [1] and want[2]["candidates"] == [0]
    assert list(bits(final)) == list(bits([0.5, 0.02]))


def test_loop_neighbour_below_min_score_still_adds():
    """passes without the feature: it asserts on the restatement"""
    want, _ = ks.reference(*order_scenes()["below_min"])
    assert want[0]["n_filtered"] == 2 and want[0]["n_scored"] == 1
    assert want[0]["acc_list"] == [(f32(f32(0.5) + f32(0.25)), 0)] and want[0]["candidates"] == [0]


def test_base_scene_is_what_the_tests_rely_on():
    """passes without the feature: the scene guarantees what the GPU tests then assume"""
    sc, queries, want, _ = sweep(0, 130)
    reloc = [w for q, w in zip(queries, want) if q["kind"] == RELOC]
    assert all(1 <= w["n_candidates"] <= 6 for w in reloc)
    assert sum(w["stale"] for w in reloc) >= 100  # the in-batch order is observable
    assert 9 in want[2]["candidates"] and want[2]["min_score"] < 1  # the loop back to the first keyframes
    alone = [ks.reference(sc, [q])[0][0] for q in queries]
    assert [w["candidates"] for w in alone] != [w["candidates"] for w in want]
    sc, queries, want, _ = edge_scene()
    assert want[0]["n_sharing"] < len(sc["kfs"]) and want[0]["words"][65] == 0 and want[0]["words"][66] == 0
    assert want[1]["n_sharing"] == 0 and want[2]["n_sharing"] > 0
    assert 30 in want[7]["candidates"] and want[7]["words"][30] == len(sc["kfs"][30]["bow"])


# ---- GPU ---------------------------------------------------------------------------------

def device_db(sc, reloc_start=None):
    import kfdb
    db = kfdb.KeyFrameDatabase([k["bow"] for k in sc["kfs"]], ks.covis_rows(sc), sc["scoring"], sc["kf_bad"],
                               sc["reloc0"] if reloc_start is None else reloc_start)
    db.add(*sc["in_db"])
    return db


def check(det, want, cand_stride, ulp=None, label=""):
    """every field of every result, the candidate rows (entries past the count untouched), d_words and d_scores"""
    import kfdb
    res = det.query_results()
    cands, wd, sc = det.candidates.cpu().numpy(), det.words.cpu().numpy(), det.scores.cpu().numpy()
    for q, (r, w) in enumerate(zip(res, want)):
        at = f"{label} query {q}"
        ints = ("n_sharing", "max_common", "min_common", "n_filtered") + (() if ulp else ("n_scored", "n_candidates"))
        assert {k: getattr(r, k) for k in ints} == {k: w[k] for k in ints}, at
        assert np.array_equal(wd[q], w["words"]), at
        if ulp:  # KL: the device log
            d = np.abs(sc[q].view(np.int32).astype(np.int64) - w["scores"].view(np.int32).astype(np.int64))
            assert d.max() <= ulp and np.array_equal(sc[q] != 0, w["scores"] != 0), at
            continue
        assert r.status == (kfdb.CAPACITY if w["n_candidates"] > cand_stride else kfdb.OK), at
        assert bits(r.min_score) == bits(w["min_score"]) and bits(r.best_acc_score) == bits(w["best_acc_score"]), at
        n = min(w["n_candidates"], cand_stride)
        assert list(cands[q, :n]) == w["candidates"][:n] and (cands[q, n:] == -1).all(), at
        assert np.array_equal(bits(sc[q]), bits(w["scores"])), at


def run(sc, queries, want, final, cand_stride=16, label=""):
    import torch
    db = device_db(sc)
    det = db.detect(queries, cand_stride, rows=True)
    torch.cuda.synchronize()
    check(det, want, cand_stride, label=label)
    assert np.array_equal(bits(db.reloc_score.cpu().numpy()[:len(final)]), bits(final)), label
    return db, det


@pytest.mark.gpu
@pytest.mark.parametrize("n_kf", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("scoring", [0, 1, 2, 4, 5])
def test_gpu_size_sweep(scoring, n_kf):
    """six relocalisation queries in one batch, and the same with two loop queries mixed in (they neither read
    nor write mRelocScore, so the relocalisation queries' expected values are the same)"""
    sc, queries, want, final = sweep(scoring, n_kf)
    run(sc, queries, want, final, label="mixed")
    pure = [i for i, q in enumerate(queries) if q["kind"] == RELOC]
    run(sc, [queries[i] for i in pure], [want[i] for i in pure], final, label="reloc")


@pytest.mark.gpu
def test_gpu_hand_built_additions():
    """an empty BowVector, keyframes the query shares nothing with, erased keyframes in covis rows and in a
    covisible list, a bad covisible, queries of 0 / 1 / 64 / 65 words, a query that is a database keyframe"""
    run(*edge_scene())


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["first_word", "add_rank", "same_best", "below_min", "stale"])
def test_gpu_order(name):
    scene, queries = order_scenes()[name]
    want, final = ks.reference(scene, queries)
    run(scene, queries, want, final)


@pytest.mark.gpu
def test_gpu_batch_semantics():
    """the batch of six equals six calls of one with the state carried over, differs from six calls that each
    start from the initial state, and a repeat run gives identical bytes"""
    import torch
    sc, rq = ks.base(0, 130)
    want, final = ks.reference(sc, rq)
    alone = [ks.reference(sc, [q])[0][0] for q in rq]
    assert [w["candidates"] for w in alone] != [w["candidates"] for w in want]  # the scene guarantees it
    db, det = run(sc, rq, want, final, label="batch")
    snap = [t.cpu().numpy().tobytes() for t in (det.results, det.candidates, det.words, det.scores, db.reloc_score)]
    db2, det2 = run(sc, rq, want, final, label="repeat")
    assert snap == [t.cpu().numpy().tobytes() for t in (det2.results, det2.candidates, det2.words, det2.scores,
                                                        db2.reloc_score)]
    carried = device_db(sc)
    for q, w in zip(rq, want):  # the state stays in the database's array between the calls
        d = carried.detect([q], 16, rows=True)
        torch.cuda.synchronize()
        check(d, [w], 16, label="carried")
    assert np.array_equal(bits(carried.reloc_score.cpu().numpy()), bits(final))
    got = []
    for q, w in zip(rq, alone):
        fresh = device_db(sc)
        d = fresh.detect([q], 16, rows=True)
        torch.cuda.synchronize()
        check(d, [w], 16, label="alone")
        got.append(d.candidate_lists()[0])
    assert got != [w["candidates"] for w in want]


def guarded(det, rows):
    """det's output tensors replaced by views into larger ones filled with a guard word"""
    import kfdb
    import torch
    keep = {}
    for name in ("results", "candidates") + (("words", "scores") if rows else ()):
        t = getattr(det, name)
        nbytes = t.numel() * t.element_size()
        big = torch.full((nbytes // 4 + 16,), GUARD, dtype=torch.int32, device=t.device)
        setattr(det, name, big[:nbytes // 4].view(t.dtype).view(t.shape))
        keep[name] = (big, nbytes // 4)
    assert ctypes.sizeof(kfdb.KfdbResult) % 4 == 0
    return keep


@pytest.mark.gpu
def test_gpu_capacity():
    import kfdb
    import torch
    sc, rq = ks.base(0, 130)
    want, final = ks.reference(sc, rq)
    assert all(w["n_candidates"] >= 2 for w in want[1:3])
    db = device_db(sc)
    det = kfdb.Detection(len(rq), db.n_kf, 1, True, db.device)
    keep = guarded(det, True)
    det.candidates.fill_(-1)
    db.detect(rq, 1, out=det)
    torch.cuda.synchronize()
    check(det, want, 1)  # the true count, the first candidate written
    assert [r.status for r in det.query_results()] == [kfdb.CAPACITY if w["n_candidates"] > 1 else kfdb.OK for w in want]
    for big, n in keep.values():
        assert (big[n:] == GUARD).all()
    assert np.array_equal(bits(db.reloc_score.cpu().numpy()), bits(final))  # CAPACITY still scores


@pytest.mark.gpu
def test_gpu_bad_job_causes_and_their_neighbours():
    """every cause ends its query alone; the good queries of the batch give what they give without them"""
    import kfdb
    import torch
    sc, rq = ks.base(0, 65)
    sc["kfs"].append({"bow": words([w for w in range(sc["n_words"]) if all(w not in q["bow"] for q in rq)][:3], 0.3),
                      "connected": set(), "best_covis": [7]})  # 65: only the last query below reads its covis row
    sc["kf_bad"], sc["reloc0"] = np.zeros(66, np.uint8), np.linspace(0, 1, 66).astype(f32)
    sc["in_db"] = list(range(66))
    lone = {"kind": RELOC, "bow": dict(sc["kfs"][65]["bow"])}
    lq = ks.loop_query(sc, 64)
    bad = [dict(rq[0], raw={"kind": 2}), dict(rq[0], raw={"kind": -1}), dict(rq[0], raw={"n_words": -1}),
           dict(rq[0], raw={"n_words": 4097}), dict(rq[0], raw={"words": None}), dict(rq[0], raw={"values": None}),
           dict(lq, connected=[3, 66]), dict(lq, connected=[-1]), dict(lq, covisible=[2, 66]), dict(lq, covisible=[-1]),
           dict(lq, raw={"connected": None}), dict(lq, raw={"covisible": None}), dict(lq, raw={"n_connected": -1}),
           dict(lq, raw={"n_covisible": -2})]
    good = [rq[1], lq, rq[2], lone, rq[3]]
    want, final = ks.reference(sc, good)
    assert want[3]["candidates"] == [65]
    queries, where = [], []
    for i, g in enumerate(good):  # good and bad interleaved
        queries += bad[3 * i:3 * i + 3] + [g]
        where.append(len(queries) - 1)
    queries += bad[15:]
    db = device_db(sc)
    det = kfdb.Detection(len(queries), db.n_kf, 16, True, db.device)
    keep = guarded(det, True)
    for t in (det.candidates, det.words, det.scores.view(torch.int32)):
        t.fill_(GUARD)
    db.detect(queries, 16, out=det)
    torch.cuda.synchronize()
    res = det.query_results()
    cands, wd, scv = det.candidates.cpu().numpy(), det.words.cpu().numpy(), det.scores.cpu().numpy()
    for q, r in enumerate(res):
        if q in where:
            continue
        assert r.status == kfdb.BAD_JOB and (r.n_sharing, r.n_scored, r.n_candidates) == (0, 0, 0), q
        assert (cands[q] == GUARD).all() and (wd[q] == GUARD).all() and (scv[q].view(np.int32) == GUARD).all(), q
    for i, q in enumerate(where):
        r, w = res[q], want[i]
        assert r.status == kfdb.OK and list(cands[q, :r.n_candidates]) == w["candidates"], q
        assert (r.n_sharing, r.max_common, r.min_common, r.n_filtered, r.n_scored) == \
            (w["n_sharing"], w["max_common"], w["min_common"], w["n_filtered"], w["n_scored"]), q
        assert bits(r.best_acc_score) == bits(w["best_acc_score"]) and bits(r.min_score) == bits(w["min_score"]), q
        assert np.array_equal(wd[q], w["words"]) and np.array_equal(bits(scv[q]), bits(w["scores"])), q
    for big, n in keep.values():
        assert (big[n:] == GUARD).all()
    assert np.array_equal(bits(db.reloc_score.cpu().numpy()), bits(final))
    # a covis row out of range: only the query that reads the row (it scores keyframe 65) is bad
    sc["kfs"][65]["best_covis"] = [66]
    db = device_db(sc)
    det = db.detect(good, 16, rows=True)
    torch.cuda.synchronize()
    assert [r.status for r in det.query_results()] == [0, 0, 0, kfdb.BAD_JOB, 0]
    want4, final4 = ks.reference(sc, good[:3] + good[4:])
    assert [c for i, c in enumerate(det.candidate_lists()) if i != 3] == [w["candidates"] for w in want4]
    assert np.array_equal(bits(db.reloc_score.cpu().numpy()), bits(final4))
    # a BowVector beyond bow_words, a database array that is NULL: every query that reads it
    sc["kfs"][65]["best_covis"] = [7]
    db = device_db(sc)
    for change in ({"n_bow_total": db.n_bow_total - 1}, {"in_db": None}, {"covis": None}, {"reloc_score": None}):
        D = db.struct()
        for k, v in change.items():
            setattr(D, k, v)
        det = db.detect([rq[0], rq[1]], 16, rows=True, struct=D)
        torch.cuda.synchronize()
        assert [r.status for r in det.query_results()] == [kfdb.BAD_JOB] * 2, change
        assert (det.candidates.cpu().numpy() == -1).all()
    assert np.array_equal(bits(db.reloc_score.cpu().numpy()), bits(sc["reloc0"]))  # nothing was scored


@pytest.mark.gpu
def test_gpu_kl_scores_within_one_ulp():
    """scoring 3 uses the device log: the integer rows are exact and d_scores is within one float ulp (the
    double agrees to 1e-12 relative, far below half a float ulp, so the rounding moves by at most one);
    candidate lists are not compared"""
    import torch
    sc, rq = ks.base(3, 65)
    want, _ = ks.reference(sc, rq)
    assert all(w["n_filtered"] > 0 for w in want)
    db = device_db(sc)
    det = db.detect(rq, 16, rows=True)
    torch.cuda.synchronize()
    check(det, want, 16, ulp=1)


FALSE = [dict(n=60, row=True, garbage=True)]
PASSES = [dict(n=300, row=True)]
NEARLY = [dict(n=270, row=True)]


@pytest.mark.gpu
def test_gpu_chain_on_one_stream():
    """ComputeBoW of the frames and the keyframes, detect with the counts read on the device, emit, SearchByBoW,
    the PnPsolver set-up and one pass of the loop on one stream with no synchronisation before the final read,
    against a RelocBurst built on the host from the downloaded candidate lists"""
    import bow
    import kfdb
    import loop
    import reloc
    import reloc_scene as rs
    import synth
    import torch
    par, leaf, desc, w = synth.synthetic_vocabulary_fast(10, 4, 5)  # reloc_scene.vocabulary()'s
    voc = bow.Vocabulary.from_arrays(10, 4, 0, 0, par, leaf, desc, w)
    nq, nc, CS = 3, 3, 4
    sc = rs.build([FALSE, PASSES, NEARLY], seed=31, n_queries=nq, oracle_bow=False)
    a = lambda k: np.array(sc[k])  # noqa: E731
    n_kf, S = nq * nc, rs.N_KP

    def tables():
        frames = reloc.Frames(a("f_kps"), a("f_desc"), None, a("K"), 0.0, rs.BOUNDS, rs.SF, a("sigma2"),
                              a("inv_level_sigma2"), rs.LOG_SF)
        kfs = loop.Keyframes(a("desc"), a("angle"), a("octave"), a("valid"), a("mp_world"), a("Tcw"), a("K"), a("sigma2"))
        search = loop.KeyframeSearch(kfs, a("kps"), a("mp_desc"), a("min_dist"), a("max_dist"), rs.BOUNDS, rs.SF,
                                     a("inv_level_sigma2"), rs.LOG_SF, a("Tcw"), a("K"))
        return frames, kfs, search
    frames, kfs, search = tables()
    dev = kfs.device
    covis = np.full((n_kf, 10), -1, np.int32)
    for k in range(n_kf):  # the candidates of one frame see each other
        covis[k, :nc - 1] = [j for j in range(k // nc * nc, k // nc * nc + nc) if j != k]
    kf_bad = np.zeros(n_kf, np.uint8)
    kf_bad[nc + 1] = 1  # a candidate of frame 1 went bad after the detection's database was built
    # everything the chain needs, allocated and uploaded before it
    tf_f, tf_k = bow.BatchTransform(nq, S, dev), bow.BatchTransform(n_kf, S, dev)
    d_frame_bow = kfdb.frame_table_device(tf_f, frames.desc, frames.angle, frames.ones, frames.counts_host, fill=False)
    d_kf_bow = kfdb.frame_table_device(tf_k, kfs.desc, kfs.angle, kfs.valid, kfs.counts_host, fill=False)
    db = kfdb.KeyFrameDatabase.from_transform(tf_k, covis, 0, kf_bad=kf_bad)
    db.add(*range(n_kf))
    queries = db.queries([{"kind": kfdb.RELOC, "device": (tf_f.bow_words.data_ptr() + 4 * S * f,
                                                          tf_f.bow_values.data_ptr() + 8 * S * f,
                                                          tf_f.bow_n.data_ptr() + 4 * f)} for f in range(nq)])
    det = kfdb.Detection(nq, n_kf, CS, False, dev)
    db.reserve(nq)
    frame_of_query = torch.arange(nq, dtype=torch.int32, device=dev)
    seeds = [500 + q for q in range(nq)]
    tabs = kfdb.RelocTables(nq, CS, seeds, dev)
    burst = reloc.RelocBurst.from_tables(frames, kfs, search, tabs)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        bow.transform_batch(voc, frames.desc, frames.counts, tf_f, 4, stream)
        bow.transform_batch(voc, kfs.desc, kfs.counts, tf_k, 4, stream)
        kfdb.set_fv_n(d_frame_bow, tf_f)
        kfdb.set_fv_n(d_kf_bow, tf_k)
        db.detect(queries, CS, stream=stream, out=det)
        db.emit_reloc(det, frame_of_query, d_kf_bow, d_frame_bow, tabs, stream)
        burst.search_by_bow(stream)
        burst.setup(stream)
        burst.relocalize(1, stream=stream)
    stream.synchronize()
    lists = det.candidate_lists()
    assert all(r.status == kfdb.OK for r in det.query_results())
    assert all(1 <= len(c) <= CS for c in lists) and any(kf_bad[k] for c in lists for k in c), lists
    # the same burst built on the host from the downloaded lists, bad keyframes dropped (Tracking.cpp:1781)
    frames2, kfs2, search2 = tables()
    frames2.compute_bow(voc)
    kfs2.compute_bow(voc)
    host = reloc.RelocBurst(frames2, kfs2, search2, [(q, [k for k in lists[q] if not kf_bad[k]], seeds[q])
                                                     for q in range(nq)])
    host.search_by_bow()
    host.setup()
    host.relocalize(1)
    torch.cuda.synchronize()
    nm, match, n_corr = burst.nmatches.cpu().numpy(), burst.match.cpu().numpy(), burst.n_correspondences()
    h_nm, h_match, h_corr = host.nmatches.cpu().numpy(), host.match.cpu().numpy(), host.n_correspondences()
    cand_tab, q_tab = tabs.candidates(), tabs.queries()
    p = 0
    for q in range(nq):
        assert (q_tab[q].first_cand, q_tab[q].n_cand) == (q * CS, len(lists[q]))
        for c in range(CS):
            e = q * CS + c
            assert cand_tab[e].frame == q
            if c < len(lists[q]) and not kf_bad[lists[q][c]]:
                assert cand_tab[e].kf == lists[q][c] == host.pairs[p][1]
                assert nm[e] == h_nm[p] and np.array_equal(match[e], h_match[p]) and n_corr[e] == h_corr[p], (q, c)
                p += 1
            else:  # unused, or a bad keyframe: no match, no solver
                assert nm[e] == 0 and n_corr[e] == -1, (q, c)
    assert p == host.n_pairs and (h_corr > 0).any()
    for q, (g, h) in enumerate(zip(burst.query_results(), host.query_results())):
        live = [k for k in lists[q] if not kf_bad[k]]
        same = ("status", "round", "calls", "verifications", "hypotheses", "draws", "n_inliers", "refined", "n_good")
        assert [getattr(g, k) for k in same] == [getattr(h, k) for k in same], q
        assert bytes(g.Tcw) == bytes(h.Tcw) and bytes(g.pnp_Tcw) == bytes(h.pnp_Tcw) and bytes(g.rng_after) == bytes(h.rng_after)
        for field in ("matched", "last_cand"):
            gi, hi = getattr(g, field), getattr(h, field)
            assert (gi < 0) == (hi < 0) and (gi < 0 or lists[q][gi] == live[hi]), (q, field)
    assert any(h.status != reloc.NO_MATCH or h.calls > 0 for h in host.query_results())
