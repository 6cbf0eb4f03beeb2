"""Scenes for tests/test_globalba.py: synth.localba_scene(n_fixed=0, kf0_local=True, ...) (every pose an
output pose, keyframe 0 fixed) and what the fixtures need beyond it -- an edge count cut to an exact
number, a pose stripped of its edges, more fixed poses."""
import functools

import numpy as np

import synth

EDGE_KEYS = ("pose_idx", "point_idx", "obs", "inv_sigma2", "outlier")


def make(n_poses, n_points, seed, n_edges=None, strip_pose=None, also_fixed=(), fix_all=False, nan_pose=None, thin=None,
         drop_mono=False, **kw):
    """n_poses poses of which pose 0 is fixed; `n_edges` keeps the first n_edges edges only (the points
    behind them are left without any), `strip_pose` removes every edge of that pose, `also_fixed` sets
    more fixed flags, `nan_pose` puts a NaN into that pose's rotation, `thin` = (fraction, point, pose)
    keeps that fraction of the edges at random, every edge of that point and of that pose, and at least
    the first two edges of every point, `drop_mono` removes the monocular edges (a scene made with stereo = 1
    still has some, where the right coordinate would leave the image)"""
    s = dict(synth.localba_scene(n_poses, 0, n_points, seed, kf0_local=True, **kw))
    keep = np.ones(len(s["obs"]), bool)
    if thin is not None:
        fraction, point, pose = thin
        keep = np.random.default_rng(seed + 7).uniform(size=len(keep)) < fraction
        keep |= (s["point_idx"] == point) | (s["pose_idx"] == pose)
        first = np.r_[True, s["point_idx"][1:] != s["point_idx"][:-1]]
        keep |= first | np.r_[False, first[:-1]]
    if n_edges is not None:
        assert n_edges <= len(keep), (n_edges, len(keep))
        keep[n_edges:] = False
    if strip_pose is not None:
        keep &= s["pose_idx"] != strip_pose
    if drop_mono:
        keep &= s["obs"][:, 2] >= 0
    for k in EDGE_KEYS:
        s[k] = np.ascontiguousarray(s[k][keep])
    s["fixed"] = s["fixed"].copy()
    for p in also_fixed:
        s["fixed"][p] = 1
    if fix_all:
        s["fixed"][:] = 1
    if nan_pose is not None:
        s["Tcw"] = s["Tcw"].copy()
        s["Tcw"][nan_pose, 1, 1] = np.nan
    return s


@functools.lru_cache(maxsize=None)
def _cached(items):
    s = make(**dict(items))
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


def scene(**kw):
    return _cached(tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in kw.items())))
