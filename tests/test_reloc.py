"""Tracking::Relocalization's candidate loop on the device
(src/Tracking.cpp:1778-1912): orbgpu_reloc_setup_batch_device and
orbgpu_relocalize_batch_device (csrc/reloc.hip) against tests/reloc_ref.py on
tests/reloc_scene.py scenes (3 lost frames x 3 candidate keyframes, 300
keypoints, SearchByBoW's rows from the CPU oracle uploaded).

CPU: the reference takes every path the loop has -- matched straight after the
first optimisation, after the first search, after the second search with
30 < nGood < 50 in between; a verification ended by nGood < 10 and one by
nadditional + nGood < 50; a pose returned through bNoMore / mBestTcw; a solver
that returns early and is called again, its last call running past
mRansacMaxIts only through the `||`; nmatches < 15; N < mRansacMinInliers; an
all-false query; monocular and stereo frames -- and every scene is decisive
(reloc_ref.decisive) before any GPU comparison.  Argument errors come before
the device; reloc.py's structs have the header's layout; the host side of the
entry points runs clean under the address and undefined-behaviour sanitizers
(tests/cpp/reloc_args_main.cpp).

GPU: every stage of a verification exact against the reference fed with the
GPU's own PnP pose bits, inlier row and previous-stage poses; the control flow
equal to the reference loop's; gathers of 63 / 64 / 65 observations; the result
independent of how the passes are split and of the batch, and repeating bit for
bit; a keyframe over capacity and a NaN-poisoned candidate end alone.

Tolerances.  The PnP pose: tests/test_pnp.py's 1e-3 on R, 1e-3 (1 + |t|max) on
t.  An optimised pose from the same start: tests/test_poseopt.py's 2 float32
ulp at scale max(1, max |Tcw|).  The final mTcw against the reference loop's
starts from PnP poses that differ by the first bound; its largest deviation
over these scenes, relative to 1 + the largest reference entry, was measured on
the MI355X (MEASURED_POSE: zero, the poses were bit-equal), and four times that
is asserted.
"""
import ctypes
import functools
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import reloc_ref as rr
import reloc_scene as rs

ROOT = Path(__file__).resolve().parent.parent
ULP = 2.0 ** -23
PNP_TOL = 1e-3
# largest |mTcw - reference| / (1 + max |reference|) of a final pose on the MI355X: on these scenes the GPU's
# PnP pose has the reference's float32 bits (both solve in double and round once), and so has every later stage
MEASURED_POSE = 0.0

FEW = [dict(n=8, row=True)]                                        # nmatches < 15: no solver
SMALL = [dict(n=16, row=True), dict(n=8, row=True, garbage=True)]  # returns a pose, nadditional + nGood < 50
BIG = [dict(n=110, row=True)]                                      # nGood >= 50 straight after the first optimisation
JUNK = [dict(n=24, row=True, garbage=True)]                        # never min_inliers: runs to its maximum, no pose
LOWN = [dict(n=22, row=True, keep=18, invalidate=12)]              # N < mRansacMinInliers: bNoMore without a draw
SEARCH1 = [dict(n=34, row=True, keep=26), dict(n=70)]              # matched after the first search
# matched after the second search: the first search keeps bins 0, 5 and 10 (14 good + 2 x 10 shifted, with
# what the row left of group 0) and drops bins 15 and 20; the shifted are outliers of the second
# optimisation (30 < nGood < 50) and keep their keypoints; the second search finds bins 15 and 20
SEARCH2 = [dict(n=26, row=True), dict(n=14, bin=0), dict(n=10, bin=5, shift_px=6.0), dict(n=10, bin=10, shift_px=6.0),
           dict(n=8, bin=15), dict(n=8, bin=20)]
DEEP = [dict(n=60, row=True, depth=2.0)]                           # stereo: PnP passes, nGood < 10
SCENES = {
    "direct": dict(cands=[FEW, SMALL, BIG], seed=21),
    "search1": dict(cands=[JUNK, SEARCH1, FEW], seed=22),
    "search2": dict(cands=[LOWN, SEARCH2, BIG], seed=23),
    "all_false": dict(cands=[JUNK, SMALL, LOWN], seed=24),
    "stereo": dict(cands=[DEEP, BIG, FEW], seed=25, stereo=True),
    # the first candidate's row thinned to exactly 63, 64 and 65 pairs in queries 0, 1 and 2
    "edges": dict(cands=[[dict(n=120, row=True)], FEW, FEW], seed=26, kp_noise=0.05, keep_by_query={0: (63, 64, 65)}),
}
SEEDS = {name: [1000 + q for q in range(3)] for name in SCENES}
LOOP_SCENES = ["direct", "search1", "search2", "all_false", "stereo"]


@functools.lru_cache(maxsize=None)
def scene(name):
    kw = dict(SCENES[name])
    if "keep_by_query" in kw:
        kw["keep_by_query"] = {c: list(v) for c, v in kw["keep_by_query"].items()}
    return rs.build(**kw)


@functools.lru_cache(maxsize=None)
def reference(name):
    """the reference loop of every query of a scene, computed once per session"""
    sc = scene(name)
    return tuple(rr.relocalize(sc, q, SEEDS[name][q]) for q in range(3))


def verifs(name):
    return [e for r in reference(name) for e in r["verifications"]]


# ---- CPU ---------------------------------------------------------------------

@pytest.mark.parametrize("name", list(SCENES))
def test_reference_is_decisive(name):
    for q, r in enumerate(reference(name)):
        assert rr.decisive(r) is None, (name, q)


def test_reference_matches_straight_after_the_first_optimisation():
    for name in ("direct", "stereo"):
        for r in reference(name):
            v = r["verifications"][-1]["v"]
            assert r["status"] == "matched" and len(v.opt) == 1 and v.n_goods[0] >= 53 and v.nadditional == [-1, -1]


def test_reference_matches_after_the_first_search():
    for r in reference("search1"):
        v = r["verifications"][-1]["v"]
        assert r["status"] == "matched" and r["matched"] == 1 and len(v.opt) == 2
        assert 13 <= v.n_goods[0] <= 47 and v.nadditional[0] > 0 and v.n_goods[1] >= 53 and v.nadditional[1] == -1


def test_reference_matches_after_the_second_search():
    for r in reference("search2"):
        v = r["verifications"][-1]["v"]
        assert r["status"] == "matched" and r["matched"] == 1 and len(v.opt) == 3
        assert 33 <= v.n_goods[1] <= 47 and v.nadditional[1] > 0 and v.n_goods[2] >= 53
        # the second optimisation's outliers kept their keypoints: the final row still holds points the
        # third optimisation then nulled, and mvbOutlier flags no slot that holds a MapPoint
        assert (v.rows[1] >= 0).sum() + v.nadditional[1] > (v.rows[2] >= 0).sum()
        assert not r["outlier"][v.rows[2] >= 0].any()


def test_reference_verifications_that_end_early():
    deep = [e for e in verifs("stereo") if e["cand"] == 0]
    assert len(deep) == 3 and all(e["v"].n_goods == [e["v"].n_good] and e["v"].n_good <= 7 for e in deep)  # nGood < 10
    assert all(e["v"].nadditional == [-1, -1] for e in deep)
    small = [e for e in verifs("direct") if e["cand"] == 1]
    assert len(small) == 3  # nadditional + nGood < 50
    assert all(len(e["v"].opt) == 1 and e["v"].nadditional[0] >= 0 and e["v"].sums[0] <= 47 for e in small)


def test_reference_returns_the_best_pose_at_bnomore_and_runs_past_the_maximum_through_the_or():
    ref = reference("all_false")
    past = 0
    for r in ref:
        assert r["status"] == "no_match" and all(r["discarded"])
        s = r["solvers"][1]
        mine = [c for c in r["calls"] if c["cand"] == 1]
        assert len(mine) >= 2 and mine[0]["returned"] and mine[0]["refined"] and not mine[0]["no_more"]
        assert mine[0]["iterations"] < s.max_its  # returned before its maximum and was called again
        last = r["verifications"][-1]
        assert last["no_more"] and not last["refined"] and last["n_inliers"] == s.best_inliers >= s.min_inliers
        end = mine[-1]
        assert end["no_more"] and end["ran"] >= 5
        past += end["iterations"] > s.max_its  # iterations only the `||` of PnPsolver.cpp:224 allowed
        junk = r["solvers"][0]
        assert junk.iterations == junk.max_its and junk.best_inliers == 0
    assert past >= 1


def test_reference_discards_before_a_solver_and_without_a_draw():
    for r in reference("direct"):
        assert r["solvers"][0] is None and r["discarded"][0]  # nmatches < 15
        assert all(c["cand"] != 0 for c in r["calls"])
    sc = scene("search2")
    for q, r in enumerate(reference("search2")):
        s = r["solvers"][0]
        assert sc["nmatches"][3 * q] >= 15 and s.N < s.min_inliers and s.iterations == 0 and r["discarded"][0]
        assert r["calls"][0] == dict(r["calls"][0], cand=0, ran=0, no_more=True, returned=False)


def test_scenes_are_monocular_and_stereo():
    assert scene("direct")["f_uright"] is None
    assert (scene("stereo")["f_uright"] >= 0).all()


def test_argument_errors_come_before_the_device():
    import reloc
    L = reloc._lib()
    p = ctypes.c_void_p(256)  # never dereferenced

    def call(nq=1, nc=1, stride=8, passes=1, resume=0, state=p, rows=p, ks=p, queries=p):
        return L.orbgpu_relocalize_batch_device(nq, queries, nc, p, p, p, ks, p, stride, p, passes, resume, state, p, p,
                                                rows, None)

    for kw in (dict(nq=-1), dict(nc=-1), dict(stride=0), dict(passes=0), dict(resume=2), dict(resume=-1),
               dict(state=None), dict(rows=None), dict(ks=None), dict(queries=None), dict(nq=1 << 20, stride=1 << 12)):
        assert call(**kw) == -1, kw  # ORBGPU_ERR_ARG, not ORBGPU_ERR_NO_DEVICE
    assert call(nq=0, state=None, rows=None, ks=None, queries=None) == 0  # nothing to do: no device needed

    def setup(nc=1, stride=8, ws=p, cands=p):
        return L.orbgpu_reloc_setup_batch_device(nc, cands, p, p, p, stride, p, ws, p, None)

    for kw in (dict(nc=-1), dict(stride=0), dict(ws=None), dict(cands=None), dict(nc=1 << 20, stride=1 << 12)):
        assert setup(**kw) == -1, kw
    assert setup(nc=0, ws=None, cands=None) == 0
    assert L.orbgpu_reloc_setup_workspace_bytes(9, 300) > 0
    assert L.orbgpu_relocalize_workspace_bytes(3, 9, 300) > 0


@pytest.fixture(scope="module")
def reloc_args_main():
    subprocess.run(["make", "-C", str(ROOT / "tests" / "cpp"), "-f", "reloc.mk"], check=True, capture_output=True)
    return ROOT / "tests" / "cpp" / "reloc_args_main"


def test_host_side_of_the_entry_points_is_clean_under_the_sanitizers(reloc_args_main):
    """argument checks and the carving of both opaque blocks from a null base, compiled for the host with
    -fsanitize=address,undefined as a program of its own"""
    r = subprocess.run([str(reloc_args_main)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout


def test_struct_layouts_equal_the_header(reloc_args_main):
    import reloc
    r = subprocess.run([str(reloc_args_main), "sizes"], capture_output=True, text=True, check=True)
    got = dict(re.findall(r"(\S+) (\d+)", r.stdout))
    want = {"orbgpu_reloc_frame": ctypes.sizeof(reloc.RelocFrame),
            "orbgpu_reloc_candidate": ctypes.sizeof(reloc.RelocCandidate),
            "orbgpu_reloc_query": ctypes.sizeof(reloc.RelocQuery),
            "orbgpu_relocalize_result": ctypes.sizeof(reloc.RelocResult),
            "orbgpu_reloc_candidate_state": ctypes.sizeof(reloc.RelocCandidateState),
            "frame.level_sigma2": reloc.RelocFrame.level_sigma2.offset,
            "result.nadditional": reloc.RelocResult.nadditional.offset,
            "result.pnp_Tcw": reloc.RelocResult.pnp_Tcw.offset,
            "result.Tcw": reloc.RelocResult.Tcw.offset,
            "result.opt": reloc.RelocResult.opt.offset,
            "result.rng_after": reloc.RelocResult.rng_after.offset,
            "state.discarded": reloc.RelocCandidateState.discarded.offset}
    assert {k: int(v) for k, v in got.items()} == want


# ---- GPU ---------------------------------------------------------------------

def _gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def burst(name, only=None, kf_counts=None, poison=None):
    """the scene's burst on the GPU; only=q: a burst of query q alone; kf_counts: the keyframes' keypoint
    counts; poison=(kf, slots): those MapPoints' positions are NaN"""
    import loop
    import reloc
    sc = scene(name)
    a = lambda k: np.array(sc[k])  # noqa: E731 (the shared scene stays untouched)
    mp = a("mp_world")
    if poison is not None:
        mp[poison[0], poison[1]] = np.nan
    frames = reloc.Frames(a("f_kps"), a("f_desc"), None if sc["f_uright"] is None else a("f_uright"), a("K"), sc["bf"],
                          rs.BOUNDS, rs.SF, a("sigma2"), a("inv_level_sigma2"), rs.LOG_SF)
    kfs = loop.Keyframes(a("desc"), a("angle"), a("octave"), a("valid"), mp, a("Tcw"), a("K"), a("sigma2"),
                         counts=kf_counts)
    ks = loop.KeyframeSearch(kfs, a("kps"), a("mp_desc"), a("min_dist"), a("max_dist"), rs.BOUNDS, rs.SF,
                             a("inv_level_sigma2"), rs.LOG_SF, a("Tcw"), a("K"))
    queries = [(f, cands, seed) for (f, cands), seed in zip(sc["queries"], SEEDS[name])]
    match, nmatches = a("match"), a("nmatches")
    if only is not None:
        queries, match, nmatches = [queries[only]], match[3 * only:3 * only + 3], nmatches[3 * only:3 * only + 3]
    return reloc.RelocBurst(frames, kfs, ks, queries, match=match, nmatches=nmatches)


def snapshot(torch, rb):
    torch.cuda.synchronize()
    return (bytes(rb.results.cpu().numpy()), bytes(rb.cand_states.cpu().numpy()), rb.query_rows().copy())


def rel_dev(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / (1.0 + np.abs(want).max()))


def T4(a):
    return np.array(a, np.float32).reshape(4, 4)


def assert_pnp_pose(got, want, where):
    got, want = T4(got), np.asarray(want, np.float64)
    assert np.abs(got[:3, :3] - want[:3, :3]).max() <= PNP_TOL, where
    assert np.abs(got[:3, 3] - want[:3, 3]).max() <= PNP_TOL * (1 + np.abs(want[:3, 3]).max()), where


@pytest.mark.gpu
def test_gpu_setup_equals_the_solver_constructors():
    torch = _gpu()
    import reloc
    for name in ("direct", "search2"):
        rb = burst(name)
        rb.setup()
        torch.cuda.synchronize()
        n_corr = rb.n_correspondences()
        for q in range(3):
            for c, s in enumerate(rr.make_solvers(scene(name), q)):
                assert n_corr[3 * q + c] == (-1 if s is None else s.N), (name, q, c)
        rb.relocalize(1)
        torch.cuda.synchronize()
        for q in range(3):
            for c, s in enumerate(rr.make_solvers(scene(name), q)):
                st = rb.candidate_states()[3 * q + c]
                if s is not None:
                    assert (st.n, st.min_inliers, st.max_iterations) == (s.N, s.min_inliers, s.max_its), (name, q, c)
    assert reloc.MIN_MATCHES == rr.MIN_MATCHES


@pytest.mark.gpu
@pytest.mark.parametrize("name", LOOP_SCENES)
def test_gpu_every_stage_of_a_verification_is_exact(name):
    """After each single pass the GPU's own PnP pose (its float bits), inlier row, the mvbOutlier it
    held before and the pose each of its optimisations left go through the CPU verification: every
    row, both nadditional, every n_good / rounds and the mvbOutlier row are equal, and each optimised
    pose is within 2 float32 ulp of the reference's from the same start."""
    torch = _gpu()
    import reloc
    sc, ref = scene(name), reference(name)
    rb = burst(name)
    rb.setup()
    seen = [0, 0, 0]
    outlier = [np.zeros(rs.N_KP, bool) for _ in range(3)]
    compared, worst = 0, 0.0
    for p in range(64):
        rb.relocalize(1, resume=p > 0)
        torch.cuda.synchronize()
        res, rows = rb.query_results(), rb.query_rows()
        for q, g in enumerate(res):
            if g.verifications == seen[q]:
                continue
            assert g.verifications == seen[q] + 1
            want = ref[q]["verifications"][seen[q]]  # the same verification of the reference loop
            seen[q] += 1
            assert (g.last_cand, g.n_inliers, g.refined) == (want["cand"], want["n_inliers"], int(want["refined"])), (p, q)
            assert_pnp_pose(g.pnp_Tcw, want["Tcw"], (name, p, q))
            np.testing.assert_array_equal(rows[q, reloc.ROW_INLIERS].astype(bool), want["vb"])
            poses = {k + 1: T4(g.opt[k].Tcw) for k in range(3) if g.opt[k].rounds > 0}
            v = rr.verify(sc, q, g.last_cand, T4(g.pnp_Tcw), rows[q, reloc.ROW_INLIERS].astype(bool), outlier[q],
                          stage_poses=poses)
            assert [o.margin >= 1e-6 for o in v.opt] == [True] * len(v.opt)
            for k in range(3):
                if k < len(v.opt):
                    o = v.opt[k]
                    assert (g.opt[k].n_good, g.opt[k].rounds) == (o.n_good, o.rounds), (name, p, q, k)
                    scale = max(1.0, float(np.abs(o.Tcw).max()))
                    dev = float(np.abs(T4(g.opt[k].Tcw).astype(np.float64) - o.Tcw.astype(np.float64)).max()) / (ULP * scale)
                    worst = max(worst, dev)
                    assert dev <= 2.0, (name, p, q, k, dev)
                else:
                    assert g.opt[k].rounds == 0 and g.opt[k].n_good == 0 and not any(g.opt[k].Tcw), (name, p, q, k)
            assert list(g.nadditional) == v.nadditional and g.n_good == v.n_good, (name, p, q)
            for k in range(3):
                np.testing.assert_array_equal(rows[q, reloc.ROW_STAGE1 + k], v.rows[k])
            np.testing.assert_array_equal(rows[q, reloc.ROW_OUTLIER].astype(bool), outlier[q])
            compared += 1
        if all(r.status != reloc.PENDING for r in res):
            break
    print(f"{name}: {compared} verifications, largest optimised-pose deviation {worst:.3f} ulp")
    assert all(r.status != reloc.PENDING for r in res)
    assert seen == [len(r["verifications"]) for r in ref] and compared > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", LOOP_SCENES)
def test_gpu_control_flow_equals_the_reference_loop(name):
    torch = _gpu()
    import orbgpu
    import ransac
    import reloc
    ref = reference(name)
    assert all(rr.decisive(r) is None for r in ref)  # the condition on the inputs
    rb = burst(name)
    rb.step(n_passes=2)
    torch.cuda.synchronize()
    res, states, rows = rb.query_results(), rb.candidate_states(), rb.query_rows()
    worst = 0.0
    for q, (g, r) in enumerate(zip(res, ref)):
        want_status = reloc.MATCHED if r["status"] == "matched" else reloc.NO_MATCH
        assert (g.status, g.matched, g.round, g.calls, g.verifications, g.hypotheses, g.draws) == \
            (want_status, r["matched"], r["round"], len(r["calls"]), len(r["verifications"]), r["hypotheses"],
             4 * r["hypotheses"]), (name, q)
        after = ransac.RandState.from_buffer_copy(bytes(g.rng_after))
        assert orbgpu.lib().orbgpu_rand_r(ctypes.byref(after)) == r["after"], (name, q)
        for c, s in enumerate(r["solvers"]):
            st = states[q * 3 + c]
            if s is None:
                assert st.n == -1 and st.discarded == 1
            else:
                assert (st.n, st.min_inliers, st.max_iterations, st.iterations, st.best_inliers, st.discarded) == \
                    (s.N, s.min_inliers, s.max_its, s.iterations, s.best_inliers, int(r["discarded"][c])), (name, q, c)
        np.testing.assert_array_equal(rows[q, reloc.ROW_OUTLIER].astype(bool), r["outlier"])
        if r["verifications"]:
            last = r["verifications"][-1]
            v = last["v"]
            assert (g.last_cand, g.n_inliers, g.refined) == (last["cand"], last["n_inliers"], int(last["refined"])), q
            assert_pnp_pose(g.pnp_Tcw, last["Tcw"], (name, q))
            assert list(g.nadditional) == v.nadditional and g.n_good == v.n_good, (name, q)
            assert [g.opt[k].n_good for k in range(len(v.opt))] == v.n_goods, (name, q)
            assert [g.opt[k].rounds for k in range(3)] == [o.rounds for o in v.opt] + [0] * (3 - len(v.opt)), (name, q)
            np.testing.assert_array_equal(rows[q, reloc.ROW_INLIERS].astype(bool), last["vb"])
            np.testing.assert_array_equal(rows[q, reloc.ROW_STAGE3], v.rows[2])
            dev = rel_dev(T4(g.Tcw), v.Tcw)
            worst = max(worst, dev)
        else:
            assert g.last_cand == -1 and not any(g.Tcw) and not any(g.pnp_Tcw) and list(g.nadditional) == [-1, -1]
            assert not rows[q, :4].any()
    print(f"{name}: final mTcw deviation {worst:.3g}")
    assert worst <= 4 * MEASURED_POSE


@pytest.mark.gpu
def test_gpu_gathers_of_63_64_65_observations():
    torch = _gpu()
    import reloc
    sc, ref = scene("edges"), reference("edges")
    assert [r["verifications"][0]["n_inliers"] for r in ref] == [63, 64, 65]  # every pair an inlier: the gather's size
    assert [len(r["verifications"][0]["v"].opt[0].gidx) for r in ref] == [63, 64, 65]
    rb = burst("edges")
    rb.setup()
    rb.relocalize(1)
    torch.cuda.synchronize()
    res, rows = rb.query_results(), rb.query_rows()
    for q, g in enumerate(res):
        want = ref[q]["verifications"][0]
        assert (g.status, g.matched, g.verifications, g.n_inliers) == (reloc.MATCHED, 0, 1, 63 + q), q
        np.testing.assert_array_equal(rows[q, reloc.ROW_INLIERS].astype(bool), want["vb"])
        outlier = np.zeros(rs.N_KP, bool)
        v = rr.verify(sc, q, 0, T4(g.pnp_Tcw), rows[q, reloc.ROW_INLIERS].astype(bool), outlier)
        assert len(v.opt[0].gidx) == 63 + q and v.opt[0].margin >= 1e-6
        assert (g.opt[0].n_good, g.opt[0].rounds, g.n_good) == (v.opt[0].n_good, v.opt[0].rounds, v.n_good), q
        np.testing.assert_array_equal(rows[q, reloc.ROW_STAGE3], v.rows[2])
        np.testing.assert_array_equal(rows[q, reloc.ROW_OUTLIER].astype(bool), outlier)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["search2", "all_false"])
def test_gpu_result_does_not_depend_on_the_split_or_the_batch_and_repeats(name):
    torch = _gpu()
    import reloc
    rb = burst(name)
    rb.setup()
    rb.relocalize(12)
    whole = snapshot(torch, rb)
    assert all(r.status != reloc.PENDING for r in rb.query_results())  # 12 passes end these scenes
    rb.relocalize(12)  # a second run from the queries' rng
    again = snapshot(torch, rb)
    rb2 = burst(name)
    rb2.setup()
    for p in range(24):
        rb2.relocalize(1, resume=p > 0)
        torch.cuda.synchronize()
        if all(r.status != reloc.PENDING for r in rb2.query_results()):
            break
    single = snapshot(torch, rb2)
    rb3 = burst(name)
    rb3.setup()
    rb3.relocalize(2)
    rb3.relocalize(3, resume=True)
    rb3.relocalize(7, resume=True)
    split = snapshot(torch, rb3)
    for a, b in ((whole, again), (whole, single), (whole, split)):
        assert a[0] == b[0] and a[1] == b[1]
        np.testing.assert_array_equal(a[2], b[2])
    nr, ns = len(whole[0]) // 3, len(whole[1]) // 3
    for q in range(3):  # nor on the batch: each query alone gives its bytes
        rb4 = burst(name, only=q)
        rb4.setup()
        rb4.relocalize(12)
        alone = snapshot(torch, rb4)
        assert alone[0] == whole[0][q * nr:(q + 1) * nr] and alone[1] == whole[1][q * ns:(q + 1) * ns], q
        np.testing.assert_array_equal(alone[2][0], whole[2][q])


@pytest.mark.gpu
def test_gpu_keyframe_over_capacity_ends_its_query_alone():
    """A candidate keyframe with one keypoint more than match_stride: the query ends with the capacity
    status before any draw (nothing is truncated), the other queries are untouched."""
    torch = _gpu()
    import reloc
    rb = burst("direct")
    rb.setup()
    rb.relocalize(4)
    whole = snapshot(torch, rb)
    counts = np.full(9, rs.N_KP, np.int32)
    counts[2] = rs.N_KP + 1  # query 0's last candidate; slot 300 is the next keyframe's first slot in HBM
    rb2 = burst("direct", kf_counts=counts)
    rb2.setup()
    rb2.relocalize(4)
    got = snapshot(torch, rb2)
    g = rb2.query_results()[0]
    assert (g.status, g.matched, g.calls, g.verifications, g.hypotheses, g.last_cand) == (reloc.CAPACITY, -1, 0, 0, 0, -1)
    assert not any(g.Tcw) and not got[2][0].any()
    nr, ns = len(whole[0]) // 3, len(whole[1]) // 3
    assert got[0][nr:] == whole[0][nr:] and got[1][ns:] == whole[1][ns:]
    np.testing.assert_array_equal(got[2][1:], whole[2][1:])


@pytest.mark.gpu
def test_gpu_nan_poisoned_candidate_ends_and_leaves_its_neighbours_alone():
    """Every MapPoint of query 0's second candidate has a NaN position: each of its PnP hypotheses is
    NaN, none has an inlier, the solver runs to its maximum (the reference's bound) and the query ends;
    the other queries' bytes are those of the clean run."""
    torch = _gpu()
    import reloc
    rb = burst("all_false")
    rb.setup()
    rb.relocalize(12)
    whole = snapshot(torch, rb)
    rb2 = burst("all_false", poison=(1, slice(None)))
    rb2.setup()
    rb2.relocalize(12)
    got = snapshot(torch, rb2)
    g, st = rb2.query_results()[0], rb2.candidate_states()[1]
    assert (g.status, g.matched, g.verifications) == (reloc.NO_MATCH, -1, 0)
    assert (st.iterations, st.best_inliers, st.discarded) == (st.max_iterations, 0, 1)
    nr, ns = len(whole[0]) // 3, len(whole[1]) // 3
    assert got[0][nr:] == whole[0][nr:] and got[1][ns:] == whole[1][ns:]
    np.testing.assert_array_equal(got[2][1:], whole[2][1:])
