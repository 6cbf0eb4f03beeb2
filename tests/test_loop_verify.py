"""The verified loop of LoopClosing::ComputeSim3 (src/LoopClosing.cpp:339-411):
orbgpu_compute_sim3_verified_batch_device (csrc/loop_verify.hip) against
tests/loop_verify_ref.py on tests/loop_verify_scene.py scenes (3 queries x 3
candidates, 300 keypoints, match12 from the CPU oracle uploaded).

CPU: the reference rejects a decoy and then matches the true candidate; a decoy
with N = 22 returns on each of its 4 iterations, the last included, and is
discarded by the empty call that follows.
GPU: every stage of a verification exact against the reference fed with the
GPU's own RANSAC Sim3 bits; the control flow (status, candidate, round,
verifications, hypotheses, draws, stream, solver states) equal to the
reference loop's; gathers of 63 / 64 / 65 correspondences; the result does not
depend on how the passes are split and repeats bit for bit; the old call and
the new agree where the first verification passes; argument errors come
before the device is looked at.

Tolerances.  The RANSAC pose: tests/test_loop.py's 2e-4.  The refined T12 and
Scw start from RANSAC poses that differ by that much; their largest deviation
from the reference over these scenes, relative to 1 + the largest reference
entry, was measured on the GPU (MEASURED_*), and four times that is asserted.
"""
import ctypes
import functools

import numpy as np
import pytest

import loop_ref
import loop_verify_ref as lvr
import loop_verify_scene as lvs
import sim3opt_ref

MARGIN = 1e-6  # tests/test_sim3opt.py's policy: a chi2 this close to th2 is a decision at the threshold
RANSAC_TOL = 2e-4
MEASURED_T12 = 3.73e-9  # largest |T12 - reference| / (1 + max |reference|) of the refined Sim3 on the MI355X
MEASURED_SCW = 9.02e-9  # the same for Scw as float[16]
MEASURED_SCW_D = 9.78e-10  # and for Scw as (q, t, s) in double
TH_NONE = 1e-3  # a SearchBySim3 radius that holds no keypoint: the gather is the RANSAC inliers alone

SCENES = {
    # unrelated / decoy / true (its BoW row thinned, so SearchBySim3 has pairs to find)
    "decoy_true": dict(inlier_frac=[0.0, 0.4, 0.4], outlier_frac=[0.1, 0.0, 0.3], decoys=(1,), keep={2: 50}, seed=11),
    # false loop / decoy with N = 22 (4 iterations, every one returns) / false loop
    "decoy_last": dict(inlier_frac=[0.0, 0.4, 0.0], outlier_frac=[0.1, 0.0, 0.3], decoys=(1,), keep={1: 22}, seed=12),
    "all_false": dict(inlier_frac=0.0, outlier_frac=[0.1, 0.2, 0.3], seed=13),
    # stereo / RGB-D: decoy, then the true loop
    "fix_scale": dict(inlier_frac=[0.4, 0.4, 0.0], outlier_frac=[0.0, 0.0, 0.3], decoys=(0,), keep={1: 50}, seed=14,
                      fix_scale=True),
    # the first verification passes
    "true_first": dict(inlier_frac=[0.4, 0.0, 0.0], outlier_frac=[0.0, 0.2, 0.3], keep={0: 60}, seed=15),
    # three decoys of exactly 63, 64 and 65 correspondences (with TH_NONE)
    "edges": dict(inlier_frac=0.4, decoys=(0, 1, 2), keep={0: 63, 1: 64, 2: 65}, seed=16),
}
SEEDS = {name: [1000 * (k + 1) + q for q in range(3)] for k, name in enumerate(SCENES)}


@functools.lru_cache(maxsize=None)
def scene(name):
    return lvs.build(3, 3, **SCENES[name])


@functools.lru_cache(maxsize=None)
def reference(name, th_search=7.5, max_verifications=None):
    """the reference loop of every query of a scene, computed once per session"""
    sc = scene(name)
    return tuple(lvr.compute_sim3_verified(sc, q, SEEDS[name][q], th_search=th_search,
                                           max_verifications=max_verifications) for q in range(3))


def decisive(ref):
    """the condition of the control-flow comparison: no verification within rounding of 20 inliers"""
    return all(v["v"].n_in <= 10 or v["v"].n_in >= 40 for r in ref for v in r["verifications"])


# ---- CPU ---------------------------------------------------------------------

def test_reference_rejects_decoy_then_matches_true():
    ref = reference("decoy_true")
    assert decisive(ref)
    for r in ref:
        assert r["status"] == "matched" and r["matched"] == 2
        log = r["verifications"]
        assert len(log) >= 2
        assert all(v["cand"] == 1 and v["v"].n_in == 0 for v in log[:-1])  # the decoy, each time it returned
        assert log[-1]["cand"] == 2 and log[-1]["v"].n_in >= 40
        assert not r["discarded"][1]  # a solver that returned stays alive
        tr = scene("decoy_true")["truth"][ref.index(r) * 3 + 2]
        S = log[-1]["v"].opt.S
        assert abs(S[2] - tr["s"]) < 0.02 and np.abs(np.array(S[1]) - tr["t"]).max() < 0.05
    # SearchBySim3 found pairs the thinned BoW row lacks
    assert sum(r["verifications"][-1]["v"].n_found for r in ref) > 0


def test_reference_decoy_returns_on_its_last_iteration_then_empty_call():
    ref = reference("decoy_last")
    assert decisive(ref)
    for r in ref:
        log = r["verifications"]
        s = r["solvers"][1]
        assert (s.N, s.max_its) == (22, 4)
        # one return per call, on the call's first iteration, in rounds 0..3: the last uses the last iteration
        assert [(v["cand"], v["round"], v["call_iterations"], v["iterations"]) for v in log] == \
            [(1, k, 1, k + 1) for k in range(4)]
        assert all(v["v"].n_in == 0 for v in log)
        assert s.iterations == s.max_its and r["discarded"][1]  # by the empty call of round 4
        assert r["status"] == "no_match" and all(r["discarded"])
        others = [x for i, x in enumerate(r["solvers"]) if i != 1 and x is not None]
        assert others and all(x.iterations == x.max_its for x in others)


def test_argument_errors_come_before_the_device():
    import loop
    L = loop._lib()
    prm = loop.Sim3RansacParams(0.99, 20, 300, 5, 0)
    p = ctypes.c_void_p(256)  # never dereferenced

    def call(nq=1, stride=8, params=prm, th=7.5, th2=10.0, mo=20, passes=1, resume=0, state=p, rows=p, ks=p):
        return L.orbgpu_compute_sim3_verified_batch_device(nq, p, 1, p, p, ks, p, stride, p, p, params, th, th2, mo,
                                                           passes, resume, state, p, p, rows, None)

    bad = [dict(nq=-1), dict(stride=0), dict(passes=0), dict(resume=2), dict(th=0.0), dict(th2=-1.0), dict(mo=-1),
           dict(state=None), dict(rows=None), dict(ks=None), dict(params=loop.Sim3RansacParams(1.5, 20, 300, 5, 0)),
           dict(params=loop.Sim3RansacParams(0.99, 20, 300, 0, 0))]
    for kw in bad:
        assert call(**kw) == -1, kw  # ORBGPU_ERR_ARG, not ORBGPU_ERR_NO_DEVICE
    assert call(nq=0, state=None, rows=None, ks=None) == 0  # nothing to do: no device needed
    assert L.orbgpu_compute_sim3_verified_workspace_bytes(3, 300) > 0


# ---- GPU ---------------------------------------------------------------------

def _gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def burst(name, only=None, counts=None, **kw):
    """the scene's burst on the GPU; only=q: a burst of query q alone; counts: the keyframes' keypoint counts"""
    import loop
    sc = scene(name)
    a = lambda k: np.array(sc[k])  # noqa: E731 (the shared scene stays untouched)
    kfs = loop.Keyframes(a("desc"), a("angle"), a("octave"), a("valid"), a("mp_world"), a("Tcw"), a("K"), a("sigma2"),
                         counts=counts)
    ks = loop.KeyframeSearch(kfs, a("kps"), a("mp_desc"), a("min_dist"), a("max_dist"), lvs.BOUNDS, lvs.SF,
                             a("inv_level_sigma2"), lvs.LOG_SF, a("Tcw"), a("K"))
    queries = [(cur, cands, seed) for (cur, cands), seed in zip(sc["queries"], SEEDS[name])]
    match12, nmatches = a("match12"), a("nmatches")
    if only is not None:
        queries, match12, nmatches = [queries[only]], match12[3 * only:3 * only + 3], nmatches[3 * only:3 * only + 3]
    return loop.LoopBurst(kfs, queries, fix_scale=sc["fix_scale"], search=ks, match12=match12, nmatches=nmatches, **kw)


def snapshot(torch, lb):
    torch.cuda.synchronize()
    return (bytes(lb.vresults.cpu().numpy()), bytes(lb.vcand_states.cpu().numpy()), lb.verified_rows().copy())


def rel_dev(got, want):
    want = np.asarray(want, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - want).max() / (1.0 + np.abs(want).max()))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["decoy_true", "fix_scale", "decoy_last"])
def test_gpu_every_stage_of_a_verification_is_exact(name):
    """After each single pass the GPU's own last RANSAC Sim3 (its float bits) and
    inlier row go through the CPU verification: SearchBySim3's row and count, the
    gathered count, the row before the removals, and -- where no chi2 is at the
    threshold -- OptimizeSim3's n_in, rounds, first nBad and the final row."""
    torch = _gpu()
    import loop
    sc = scene(name)
    ref = reference(name)
    lb = burst(name)
    lb.setup()
    seen = [0, 0, 0]
    compared = decided = 0
    for p in range(12):
        lb.compute_sim3_verified(1, resume=p > 0)
        torch.cuda.synchronize()
        res, rows = lb.verified_results(), lb.verified_rows()
        for q, r in enumerate(res):
            if r.verifications == seen[q]:
                continue
            assert r.verifications == seen[q] + 1
            want = ref[q]["verifications"][seen[q]]  # the same verification of the reference loop
            seen[q] += 1
            assert r.last_cand == want["cand"] and r.n_inliers == want["n_inliers"]
            np.testing.assert_allclose(np.array(r.R12).reshape(3, 3), want["pose"]["R12"], atol=RANSAC_TOL)
            assert abs(r.s12 - want["pose"]["s12"]) < RANSAC_TOL
            np.testing.assert_allclose(np.array(r.t12), want["pose"]["t12"],
                                       atol=RANSAC_TOL * (1 + np.abs(want["pose"]["t12"]).max()))
            np.testing.assert_array_equal(rows[q, 0].astype(bool), want["vb"])
            v = lvr.verify(sc, q, r.last_cand, np.array(r.R12, np.float32), np.array(r.t12, np.float32),
                           np.float32(r.s12), rows[q, 0].astype(bool))
            np.testing.assert_array_equal(rows[q, 1], v.agreed)
            assert r.n_found == v.n_found
            assert r.n_gathered == len(v.gidx)
            m_search = np.where(rows[q, 1] >= 0, rows[q, 1], np.where(rows[q, 0] > 0, sc["match12"][q * 3 + r.last_cand], -1))
            np.testing.assert_array_equal(m_search, v.m_search)
            # the removals only ever clear gathered slots, in the gather's order
            assert set(np.nonzero(rows[q, 2] != m_search)[0]) <= set(v.gidx.tolist())
            compared += 1
            print(f"{name} q{q} cand {r.last_cand}: found {r.n_found} gathered {r.n_gathered} nIn {r.opt.n_in} "
                  f"(ref {v.opt.n_in}) margin {sim3opt_ref.threshold_margin(v.opt, 10.0):.3g}")
            if sim3opt_ref.threshold_margin(v.opt, 10.0) >= MARGIN:
                decided += 1
                assert (r.opt.n_in, r.opt.rounds, r.opt.n_bad_first) == (v.opt.n_in, v.opt.rounds, v.opt.n_bad_first)
                np.testing.assert_array_equal(rows[q, 2], v.m)
        if all(r.status != loop.PENDING for r in res):
            break
    assert all(r.status != loop.PENDING for r in res)
    assert seen == [len(r["verifications"]) for r in ref]
    assert compared > 0 and decided > 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["decoy_true", "decoy_last", "all_false", "fix_scale"])
def test_gpu_control_flow_equals_the_reference_loop(name):
    torch = _gpu()
    import loop
    import orbgpu
    import ransac
    ref = reference(name)
    assert decisive(ref)  # the condition on the inputs: no decision within rounding of 20
    lb = burst(name)
    lb.step_verified(n_passes=2)
    torch.cuda.synchronize()
    res, states = lb.verified_results(), lb.verified_candidate_states()
    worst_t12 = worst_scw = worst_scw_d = 0.0
    for q, (g, r) in enumerate(zip(res, ref)):
        want_status = loop.MATCHED if r["status"] == "matched" else loop.NO_MATCH
        assert (g.status, g.matched, g.round, g.verifications, g.hypotheses, g.draws) == \
            (want_status, r["matched"], r["round"], len(r["verifications"]), r["hypotheses"], 3 * r["hypotheses"]), q
        after = ransac.RandState.from_buffer_copy(bytes(g.rng_after))
        assert orbgpu.lib().orbgpu_rand_r(ctypes.byref(after)) == r["after"], q
        for c, s in enumerate(r["solvers"]):
            st = states[q * 3 + c]
            if s is None:
                assert st.n == -1 and st.discarded == 1
            else:
                assert (st.n, st.max_iterations, st.iterations, st.best_inliers, st.discarded) == \
                    (s.N, s.max_its, s.iterations, s.best, int(r["discarded"][c])), (q, c)
        if r["verifications"]:
            last = r["verifications"][-1]
            assert (g.last_cand, g.n_inliers, g.n_found, g.n_gathered) == \
                (last["cand"], last["n_inliers"], last["v"].n_found, len(last["v"].gidx)), q
            assert (g.opt.n_in, g.opt.rounds) == (last["v"].opt.n_in, last["v"].opt.rounds), q
            if last["v"].opt.rounds == 2:
                worst_t12 = max(worst_t12, rel_dev(np.array(g.opt.T12).reshape(4, 4), last["v"].opt.T12))
        if r["status"] == "matched":
            worst_scw = max(worst_scw, rel_dev(np.array(g.Scw).reshape(4, 4), r["Scw_T"]))
            Sq, St, Ss = r["Scw"]
            worst_scw_d = max(worst_scw_d, rel_dev(list(g.Scw_q) + list(g.Scw_t) + [g.Scw_s], list(Sq) + list(St) + [Ss]))
        else:  # no match: the pose words are zero
            assert not any(g.Scw) and not any(g.Scw_q) and not any(g.Scw_t) and g.Scw_s == 0.0
    print(f"{name}: refined T12 deviation {worst_t12:.3g}, Scw deviation {worst_scw:.3g} (float), "
          f"{worst_scw_d:.3g} (double)")
    assert worst_t12 <= 4 * MEASURED_T12
    assert worst_scw <= 4 * MEASURED_SCW
    assert worst_scw_d <= 4 * MEASURED_SCW_D


@pytest.mark.gpu
def test_gpu_gathers_of_63_64_65_correspondences():
    torch = _gpu()
    sc = scene("edges")
    ref = reference("edges", TH_NONE, 3)
    for r in ref:  # every decoy returns at once with all its correspondences, and fails
        assert [len(v["v"].gidx) for v in r["verifications"][:3]] == [63, 64, 65]
    lb = burst("edges", th_search=TH_NONE)
    lb.setup()
    for p in range(3):
        lb.compute_sim3_verified(1, resume=p > 0)
        torch.cuda.synchronize()
        res, rows = lb.verified_results(), lb.verified_rows()
        for q, g in enumerate(res):
            want = ref[q]["verifications"][p]
            assert (g.last_cand, g.verifications, g.n_found, g.n_gathered) == (p, p + 1, 0, 63 + p), (p, q)
            v = lvr.verify(sc, q, p, np.array(g.R12, np.float32), np.array(g.t12, np.float32), np.float32(g.s12),
                           rows[q, 0].astype(bool), th_search=TH_NONE)
            np.testing.assert_array_equal(rows[q, 0].astype(bool), want["vb"])
            assert len(v.gidx) == 63 + p
            if sim3opt_ref.threshold_margin(v.opt, 10.0) >= MARGIN:
                assert (g.opt.n_in, g.opt.rounds, g.opt.n_bad_first) == (v.opt.n_in, v.opt.rounds, v.opt.n_bad_first)
                np.testing.assert_array_equal(rows[q, 2], v.m)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["decoy_true", "decoy_last"])
def test_gpu_result_does_not_depend_on_the_split_or_the_batch_and_repeats(name):
    torch = _gpu()
    import loop
    lb = burst(name)
    lb.setup()
    lb.compute_sim3_verified(8)
    whole = snapshot(torch, lb)
    assert all(r.status != loop.PENDING for r in lb.verified_results())  # 8 passes end these scenes
    lb.compute_sim3_verified(8)  # a second run from the queries' rng
    again = snapshot(torch, lb)
    lb2 = burst(name)
    lb2.setup()
    for p in range(16):
        lb2.compute_sim3_verified(1, resume=p > 0)
        torch.cuda.synchronize()
        if all(r.status != loop.PENDING for r in lb2.verified_results()):
            break
    single = snapshot(torch, lb2)
    for a, b in ((whole, again), (whole, single)):
        assert a[0] == b[0] and a[1] == b[1]
        np.testing.assert_array_equal(a[2], b[2])
    # nor on the batch: query 1 alone gives query 1's bytes
    lb3 = burst(name, only=1)
    lb3.setup()
    lb3.compute_sim3_verified(8)
    alone = snapshot(torch, lb3)
    nr, ns = len(alone[0]), len(alone[1])
    assert alone[0] == whole[0][nr:2 * nr] and alone[1] == whole[1][ns:2 * ns]
    np.testing.assert_array_equal(alone[2][0], whole[2][1])


@pytest.mark.gpu
def test_gpu_old_and_new_calls_agree_where_the_first_verification_passes():
    torch = _gpu()
    import loop
    ref = reference("true_first")
    assert all(r["status"] == "matched" and len(r["verifications"]) == 1 for r in ref)
    lb = burst("true_first")
    lb.setup()
    lb.compute_sim3()
    lb.compute_sim3_verified(1)
    torch.cuda.synchronize()
    old, new, rows = lb.query_results(), lb.verified_results(), lb.verified_rows()
    for q in range(3):
        o, n = old[q], new[q]
        assert n.status == loop.MATCHED
        assert (n.matched, n.round, n.hypotheses, n.draws, n.n_inliers) == \
            (o.matched, o.round, o.hypotheses, o.draws, o.n_inliers)
        assert bytes(n.R12) == bytes(o.R12) and bytes(n.t12) == bytes(o.t12) and bytes(n.T12) == bytes(o.T12)
        assert np.float32(n.s12).tobytes() == np.float32(o.s12).tobytes()
        assert bytes(n.rng_after) == bytes(o.rng_after)
        np.testing.assert_array_equal(rows[q, 0].astype(bool), lb.vb_inliers(q, old))


@pytest.mark.gpu
def test_gpu_keyframe_over_capacity_ends_its_query_alone():
    """A candidate with one keypoint more than match_stride: the projection
    matcher rejects the call (nothing is truncated), the query ends with the
    capacity status at its first verification, the other queries are untouched."""
    torch = _gpu()
    import loop
    lb = burst("true_first")
    lb.setup()
    lb.compute_sim3_verified(2)
    whole = snapshot(torch, lb)
    counts = np.full(12, 300, np.int32)
    counts[3] = 301  # query 0's first candidate; slot 300 is the next keyframe's first slot in HBM
    lb2 = burst("true_first", counts=counts)
    lb2.setup()
    lb2.compute_sim3_verified(2)
    got = snapshot(torch, lb2)
    g = lb2.verified_results()[0]
    assert (g.status, g.matched, g.verifications, g.last_cand) == (loop.CAPACITY, -1, 0, 0)
    assert not any(g.Scw) and not any(g.Scw_q) and g.Scw_s == 0.0
    nr = len(whole[0]) // 3
    assert got[0][nr:] == whole[0][nr:]
    np.testing.assert_array_equal(got[2][1:], whole[2][1:])
