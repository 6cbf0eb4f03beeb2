"""Projection matchers on constructed scenes (tests/proj_cases.py): the walk's rescans, same-batch
conflicts and repeated assignments, every threshold from both sides, ties, grid and capacity edges,
the rotation cull, isInFrustum and a multi-call launch.  Bar, as in test_proj.py / test_fuse.py:
the count and every match entry equal to the Python oracle's (oracle/proj_ref.py).

The CPU tests run the builders, whose own assertions make sure each scene reaches its edge, and
hold the C++ restatement (oracle/proj_ref.cpp) against the Python one on every LOCAL and
LAST_FRAME scene."""
import numpy as np
import pytest

import proj_cases as pc
import proj_ref

FAMILIES = sorted(pc.FAMILIES)


@pytest.mark.parametrize("family", FAMILIES)
def test_builders_reach_their_edges(family):
    """the builders assert it; here: every family is there, and its scenes are distinct"""
    scenes = pc.FAMILIES[family]()
    assert len(scenes) >= 7
    assert all(name == sc["name"] for name, sc in scenes.items())


def test_stacked_census():
    fam = pc.stacked_family()
    for v in pc.WALKERS:
        c = fam[f"stacked/{pc.NAMES[v]}"]["census"]
        assert c["queries"] == 432 and c["conflicts"] == 378 and c["max_cands"] == 8
        assert c["rescans"] == (270 if v == pc.LOCAL else 216)
        assert sum(ip < pc.CHUNK for ip in c["rescan_points"]) >= 100
        c = fam[f"stacked-drop5/{pc.NAMES[v]}"]["census"]
        assert {63, 64, 240} <= set(c["rescan_points"])
        assert fam[f"stacked-interleaved/{pc.NAMES[v]}"]["census"]["conflicts"] < 50
    c = fam["stacked-noobs-ori/last"]["census"]
    assert c["twice"] == 54 and c["two_bins"] >= 5 and c["culled_kept"] >= 1
    assert fam["stacked-noobs-ori/last"]["expect"][0] == 432 - 22
    assert fam["stacked-noobs/local"]["census"]["twice"] >= 40


def test_census_counts_a_hand_made_trace():
    """two points of one batch on one slot list: the second finds its best hidden by the first"""
    rec = lambda ip, hidden, slot, b: {"ip": ip, "cands": [0, 1, 2, 3, 4], "hidden": hidden, "slot": slot, "bin": b,
                                       "passed": [(i, 10 * i, 0) for i in range(5)]}
    tgt = {"kps": np.zeros(5), "occupied": None}
    pts = {"flags": np.full(300, pc.VALID | pc.HAS_OBS, np.int32)}
    trace = [rec(0, [], 0, 3), rec(1, [0], 1, 3), rec(2, [0, 1], 2, 4), rec(3, [0, 1, 2], 3, 3),
             rec(64, [0, 1, 2, 3], 4, 3), rec(65, [0, 1, 2, 3, 4], None, None)]
    c = pc.census(trace, pc.KEYFRAME, tgt, pts)
    assert (c["rescans"], c["rescan_points"], c["conflicts"], c["twice"], c["max_cands"]) == (2, [64, 65], 3, 0, 5)
    assert (c["two_bins"], c["culled"], c["culled_kept"]) == (0, 0, 0)
    c = pc.census(trace, pc.LOCAL, tgt, pts)  # needs two visible entries: point 3 sees one of the four
    assert c["rescan_points"] == [3, 64, 65]
    again = [rec(0, [], 0, 3), rec(1, [], 0, 9), rec(2, [], 0, 3), rec(3, [], 1, 3)]
    c = pc.census(again, pc.LAST_FRAME, tgt, {"flags": np.full(4, pc.VALID, np.int32)})
    assert (c["twice"], c["two_bins"], c["culled"], c["culled_kept"], c["conflicts"]) == (1, 1, 0, 0, 0)
    again += [rec(4 + i, [], 2 + i % 2, 3) for i in range(18)]  # bin 3 grows to 21 entries: bin 9's one is culled
    c = pc.census(again, pc.LAST_FRAME, tgt, {"flags": np.full(22, pc.VALID, np.int32)})
    assert (c["culled"], c["culled_kept"]) == (1, 1)


def test_trace_does_not_change_the_oracle():
    sc = pc.stacked_family()["stacked-ori/kf"]
    nm, m = proj_ref.search_by_projection(sc["variant"], sc["tgt"], sc["pts"], sc["th"], **sc["kw"])
    assert nm == sc["expect"][0] and np.array_equal(m, sc["expect"][1])
    sc = pc.ties_family()["tie-two-columns-d7/fuse"]
    nm, m = proj_ref.radius_search(sc["variant"], sc["tgt"], sc["pts"], sc["th"])
    assert nm == sc["expect"][0] and np.array_equal(m, sc["expect"][1])


@pytest.mark.parametrize("family", FAMILIES)
def test_cpp_oracle_equals_python_oracle(family):
    """orbref.search_by_projection (LOCAL, LAST_FRAME) on every such scene"""
    import orbref
    bad = []
    for name, sc in pc.FAMILIES[family]().items():
        if sc["variant"] not in (pc.LOCAL, pc.LAST_FRAME):
            continue
        nm, m = orbref.search_by_projection(sc["variant"], sc["tgt"], sc["pts"], sc["th"], **sc["kw"])
        if nm != sc["expect"][0] or not np.array_equal(m, sc["expect"][1]):
            bad.append((name, nm, sc["expect"][0], np.nonzero(m != sc["expect"][1])[0][:8]))
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("family", FAMILIES)
def test_gpu_scenes_exact(family):
    import proj
    bad = []
    for name, sc in pc.FAMILIES[family]().items():
        nm, m = proj.search_by_projection(sc["variant"], sc["tgt"], sc["pts"], sc["th"], **sc["kw"])
        if nm != sc["expect"][0] or not np.array_equal(m, sc["expect"][1]):
            diff = np.nonzero(m != sc["expect"][1])[0]
            bad.append((name, nm, sc["expect"][0], diff[:8], m[diff[:8]], sc["expect"][1][diff[:8]]))
    assert not bad, (len(bad), bad[:10])


@pytest.mark.gpu
def test_gpu_is_in_frustum_edges():
    import proj
    tgt, pts, cos_limit, (fr, tr, lr) = pc.frustum_case()
    n = len(fr)
    assert n == 257 and (pts["flags"] & pc.IN_VIEW).all()
    track0 = np.arange(4 * n, dtype=np.float32).reshape(n, 4) - 1000.5
    level0 = np.arange(n, dtype=np.int32) - 77
    fg, tg, lg = proj.is_in_frustum(tgt, pts, cos_limit, track0=track0, level0=level0)
    np.testing.assert_array_equal(fg, fr)
    inv = (fr & pc.IN_VIEW) != 0
    np.testing.assert_array_equal(lg[inv], lr[inv])
    np.testing.assert_array_equal(tg[inv].view(np.uint32), tr[inv].view(np.uint32))
    np.testing.assert_array_equal(lg[~inv], level0[~inv])
    np.testing.assert_array_equal(tg[~inv].view(np.uint32), track0[~inv].view(np.uint32))


def _call(sc):
    return dict(variant=sc["variant"], tgt=sc["tgt"], pts=sc["pts"], th=sc["th"], **sc["kw"])


def _batch_scenes():
    st, ties, cap = pc.stacked_family(), pc.ties_family(), pc.capacity_family()
    grid, rot, depth = pc.grid_family(), pc.rotation_family(), pc.depth_family()
    good = [st["stacked-cut241/local"], st["stacked-cut65/sim3"], st["stacked-noobs-ori/last"], st["stacked-ori/kf"],
            grid["grid-edges/fuse"], depth["negative-depth/fusesim3"], ties["tie-two-columns-d7/sim3dir"],
            st["stacked-five/kf"], rot["rot-bins/last"], cap["capacity-1/sim3"]]
    empty_target = pc.scene("empty-target", pc.KEYFRAME, pc.make_target(np.zeros((0, 2)), np.zeros((0, 32))),
                            st["stacked-cut63/kf"]["pts"])
    nothing = {k: v[:0] for k, v in st["stacked-cut63/sim3"]["pts"].items()}
    empty_points = pc.scene("empty-points", pc.SIM3, st["stacked-cut63/sim3"]["tgt"], nothing)
    return good + [empty_target, empty_points]


@pytest.mark.gpu
def test_gpu_batch_launch():
    """twelve good calls of all seven variants, an over-capacity target and a call whose row does not fit
    the stride, in one launch"""
    import proj
    good = _batch_scenes()
    assert {sc["variant"] for sc in good} == set(pc.ALL)
    nout = [len(sc["pts"]["flags"]) if sc["variant"] in pc.PER_POINT else len(sc["tgt"]["kps"]) for sc in good]
    stride = max(nout) + 5
    rng = np.random.default_rng(16)
    big = pc.make_target(rng.uniform(0, 640, (4097, 2)), rng.integers(0, 256, (4097, 32), dtype=np.uint8))
    over = dict(_call(good[3]), tgt=big)  # 4097 keypoints
    wide = pc.make_target(rng.uniform(0, 640, (stride + 1, 2)), rng.integers(0, 256, (stride + 1, 32), dtype=np.uint8))
    assert stride + 1 <= 4096
    too_wide = dict(_call(good[1]), tgt=wide)  # n > stride
    calls = [_call(sc) for sc in good]
    calls[5:5] = [over]
    calls.append(too_wide)
    rejected = {5, len(calls) - 1}
    nm, match = proj.search_by_projection_batch(calls, stride, fill=-7)
    assert match.shape == (len(calls), stride) and len(calls) >= 9
    it = iter(zip(good, nout))
    for c in range(len(calls)):
        if c in rejected:
            assert nm[c] == -1 and (match[c] == -7).all(), c
            continue
        sc, n = next(it)
        assert nm[c] == sc["expect"][0], (c, sc["name"])
        np.testing.assert_array_equal(match[c, :n], sc["expect"][1], err_msg=sc["name"])
        assert (match[c, n:] == -7).all(), (c, sc["name"])
    assert len({len(sc["tgt"]["kps"]) for sc in good}) > 4 and len({len(sc["pts"]["flags"]) for sc in good}) > 4


@pytest.mark.gpu
def test_gpu_host_call_rejects_4097_keypoints():
    import orbgpu
    import proj
    sc = pc.stacked_family()["stacked-cut63/kf"]
    rng = np.random.default_rng(17)
    big = pc.make_target(rng.uniform(0, 640, (4097, 2)), rng.integers(0, 256, (4097, 32), dtype=np.uint8))
    with pytest.raises(orbgpu.OrbGpuError) as e:
        proj.search_by_projection(sc["variant"], big, sc["pts"], sc["th"], **sc["kw"])
    assert e.value.code == orbgpu.ERR_ARG
