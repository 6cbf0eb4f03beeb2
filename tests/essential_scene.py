"""Seeded loops for the essential-graph tests (tests/test_essential.py): a chain of
keyframes round a circle whose estimates drift (rotation, translation and, when
the scale is free, scale), the last `n_corrected` of them "corrected" by the
Sim3 that closes the loop, as LoopClosing::CorrectLoop leaves them before
Optimizer::OptimizeEssentialGraph, with spanning-tree, covisibility, loop and
LoopConnections edges and MapPoints with reference keyframes.  The arrays are
those of include/orbgpu_essential.h.
"""
import numpy as np

F32 = np.float32


def rot(w):
    """Rodrigues: the rotation matrix of the rotation vector w"""
    w = np.asarray(w, np.float64)
    th = float(np.linalg.norm(w))
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def quat(R):
    """unit quaternion (x, y, z, w) of a rotation matrix, w >= 0"""
    w = np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2])) / 2
    if w > 1e-6:
        q = np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(max(0.0, 1 + R[i, i] - R[j, j] - R[k, k])) * 2
        q = np.zeros(4)
        q[i], q[j], q[k], q[3] = s / 4, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s, (R[k, j] - R[j, k]) / s
    return q / np.linalg.norm(q)


def sim3_row(R, t, s):
    return np.concatenate([quat(R), np.asarray(t, np.float64), [s]])


def scene(n_kf, seed, fix_scale=1, n_corrected=3, drift_rot=0.01, drift_t=0.05, drift_s=0.02, fixed=(0,), covis=0.6,
          n_loop_conn=2, old_loop=True, n_edges=None, star=None, strip=None, n_points=12, no_ref=0.25, c_only=(),
          nc_only=(), start=0.0, consistent=False, nan_pose=None, multi=(), lead=()):
    """A dict of the arrays of the C ABI plus fix_scale.

    n_corrected  the last keyframes, with a corrected and a non-corrected Sim3 each
    c_only       keyframes (not among the last) with a corrected Sim3 alone; nc_only: a non-corrected alone
    fixed        the fixed keyframes (the adapter fixes pLoopKF only)
    covis        probability of each covisibility edge (k, k - 2), (k, k - 3)
    n_loop_conn  LoopConnections edges (kind 0) from corrected keyframes to the first ones
    old_loop     a loop edge of an earlier loop, (n_kf // 2 + 1, 1) of kind 1
    n_edges      exactly this many edges: the list is cut, or random pairs of either kind are added
    star         (v, count): edges between v and the others are added, both ways round, until v has count
    strip        a keyframe all of whose edges are removed
    lead         edges (i, j, kind) put before every other
    multi        tuples (a, b, n): n more edges between a and b, alternating orientation and kind
    start        a far start: the non-corrected keyframes' poses moved by this much (rad, and 3x in metres)
    consistent   the corrected Sim3s equal the non-corrected ones: nothing to optimise
    """
    rng = np.random.default_rng(seed)
    fix_scale = int(bool(fix_scale))
    # the truth: a circle of radius 5, cameras turning with it
    Rs, ts = [], []
    for k in range(n_kf):
        a = 2 * np.pi * k / max(n_kf, 1) * 0.97
        Rwc = rot([0, a, 0]) @ rot(0.05 * rng.standard_normal(3))
        c = np.array([5 * np.sin(a), 0.1 * rng.standard_normal(), 5 - 5 * np.cos(a)])
        Rs.append(Rwc.T), ts.append(-Rwc.T @ c)
    # the drifted estimates: the relative motions, each a little off, chained from keyframe 0
    Rd, td, sd = [Rs[0]] if n_kf else [], [ts[0]] if n_kf else [], [1.0] if n_kf else []
    for k in range(1, n_kf):
        Rrel = Rs[k] @ Rs[k - 1].T
        trel = ts[k] - Rrel @ ts[k - 1]
        s = sd[-1] * (1.0 if fix_scale else float(np.exp(drift_s * rng.standard_normal())))
        Rrel = rot(drift_rot * rng.standard_normal(3)) @ Rrel
        trel = s * trel + drift_t * rng.standard_normal(3)
        Rd.append(Rrel @ Rd[-1]), td.append(trel + Rrel @ td[-1]), sd.append(s)
    Tcw = np.zeros((n_kf, 3, 4))
    for k in range(n_kf):
        Tcw[k, :, :3], Tcw[k, :, 3] = Rd[k], td[k]
    has_c, has_nc = np.zeros(n_kf, np.uint8), np.zeros(n_kf, np.uint8)
    Sc, Snc = np.zeros((n_kf, 8)), np.zeros((n_kf, 8))
    Sc[:, 3] = Snc[:, 3] = Sc[:, 7] = Snc[:, 7] = 1.0
    n_corrected = min(n_corrected, max(n_kf - 1, 0))
    if n_corrected:
        last = n_kf - 1
        # the loop's Sim3 of the last keyframe: the truth, at the scale the drift reached
        s_last = 1.0 if fix_scale else 1.0 / sd[last]
        Rl, tl = Rs[last], ts[last]
        for k in range(n_kf - n_corrected, n_kf):
            Rrel = Rd[k] @ Rd[last].T                       # Sic = Siw * Swc
            trel = td[k] - Rrel @ td[last]
            has_c[k] = has_nc[k] = 1
            Snc[k] = sim3_row(Rd[k], td[k], 1.0)
            if consistent:
                Sc[k] = Snc[k]
                continue
            Sc[k] = sim3_row(Rrel @ Rl, Rrel @ tl + trel, s_last)  # Sic * the corrected Scw
            Tcw[k, :, :3], Tcw[k, :, 3] = Rrel @ Rl, (Rrel @ tl + trel) / s_last
    for k in c_only:
        has_c[k] = 1
        Sc[k] = sim3_row(rot(0.02 * rng.standard_normal(3)) @ Rd[k], td[k] + 0.05 * rng.standard_normal(3),
                         1.0 if fix_scale else 1.03)
    for k in nc_only:
        has_nc[k] = 1
        Snc[k] = sim3_row(rot(0.02 * rng.standard_normal(3)) @ Rd[k], td[k] + 0.05 * rng.standard_normal(3), 1.0)
    if start:
        for k in range(1, n_kf - n_corrected):
            if k in c_only:
                continue
            Tcw[k, :, :3] = rot(start * rng.standard_normal(3)) @ Tcw[k, :, :3]
            Tcw[k, :, 3] += 3 * start * rng.standard_normal(3)
            if not has_nc[k]:  # the measurements come from where the keyframes were
                has_nc[k] = 1
                Snc[k] = sim3_row(Rd[k], td[k], 1.0)
    fx = np.zeros(n_kf, np.uint8)
    fx[[f for f in fixed if f < n_kf]] = 1
    edges = [tuple(e) for e in lead]  # (i, j, kind)
    for c in range(min(n_loop_conn, n_corrected)):  # LoopConnections
        edges.append((n_kf - 1 - c, c, 0))
    for k in range(1, n_kf):                        # the spanning tree
        edges.append((k, k - 1, 1))
    if old_loop and n_kf > 6:
        edges.append((n_kf // 2 + 1, 1, 1))
    for k in range(2, n_kf):                        # covisibility
        for back in (2, 3):
            if k - back >= 0 and rng.uniform() < covis:
                edges.append((k, k - back, 1))
    for a, b, n in multi:
        for m in range(n):
            i, j = (a, b) if m % 2 == 0 else (b, a)
            edges.append((i, j, (m // 2) % 2))
    if star is not None:
        v, count = star
        have = sum(1 for i, j, _ in edges if v in (i, j))
        o = 0
        while have < count:
            other = (v + 1 + o % (n_kf - 1)) % n_kf
            edges.append((v, other, 1) if o % 2 == 0 else (other, v, o // 2 % 2))
            have, o = have + 1, o + 1
    if strip is not None:
        edges = [e for e in edges if strip not in e[:2]]
    if n_edges is not None:
        edges = edges[:n_edges]
        while len(edges) < n_edges:
            i, j = rng.choice(n_kf, 2, replace=False)
            if strip in (i, j):
                continue
            edges.append((int(i), int(j), int(rng.integers(0, 2))))
    e = np.array(edges, np.int64).reshape(-1, 3)
    Xw = (rng.uniform(-6, 6, (n_points, 3)) + [0, 0, 5]).astype(F32)
    ref = rng.integers(0, max(n_kf, 1), n_points).astype(np.int32)
    ref[rng.uniform(size=n_points) < no_ref] = -1
    if n_kf == 0:
        ref[:] = -1
    elif n_points >= 3:  # every scene has a point without a reference, one of a corrected and one of an uncorrected keyframe
        ref[:3] = (-1, n_kf - 1, 0)
    T32 = Tcw.reshape(n_kf, 12).astype(F32)
    if nan_pose is not None:
        T32[nan_pose, 3] = np.nan
    return dict(Tcw=T32, has_corrected=has_c, Scorrected=Sc, has_noncorrected=has_nc, Snoncorrected=Snc, fixed=fx,
                edge_i=e[:, 0].astype(np.int32), edge_j=e[:, 1].astype(np.int32), edge_kind=e[:, 2].astype(np.uint8),
                Xw=Xw, point_ref=ref, fix_scale=fix_scale)
