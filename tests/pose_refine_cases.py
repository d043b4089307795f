"""The numpy restatement, the record and the cases that tests/test_pose_refine_host.py (CPU) and tests/test_gpu_pose_refine.py (device) share.
No GPU is touched here.

refine6_np is lii_pose_refine's definition in numpy on the oracle's own pass (Tree.iterate_once): the iterated update of
src/laserMapping.cpp:957-1134 in LO mode on the six pose states, `updates` times in a row.  test_pose_refine_host.py pins it to the
oracle's 24-state Tree.iekf_update; the device tests are held to it.
"""
import numpy as np

import pose_score_cases as psc

# struct lii_pose_refined (408 bytes)
RECORD_DTYPE = np.dtype([("pose", "<f8", (12,)), ("cov", "<f8", (6, 6)), ("total_residual", "<f8"), ("effect_num", "<i4"),
                         ("iterations", "<i4"), ("searches", "<i4"), ("flags", "<i4")])
CONVERGED, BAD_POSE = 1, 2
SCHEDULES = ((4, 2), (5, 1))  # (max_iterations, updates)
# the project's update tolerance (tests/test_gpu_register.py): position, rotation; the covariance relative to its largest entry
TOL_P, TOL_R, TOL_COV = 1e-6, 1e-7, 1e-6


def unpack6(out91):
    """The pose block of a pass's 91 sums: G (6, 6) from the upper triangle of the 12 x 12 block (78, row by row), g from the z column
    (78 .. 83), effect_num (90)."""
    G = np.zeros((6, 6))
    for i in range(6):
        for j in range(i, 6):
            G[i, j] = G[j, i] = out91[i * 12 - (i * (i - 1)) // 2 + (j - i)]
    return G, out91[78:84].copy(), int(out91[90])


def refine6_np(O, tree, scan, st0, max_it, updates, prior=None, info=None):
    """(state, iterations per update, effect_num of the last pass).  `info` (a dict) also receives searches, total_residual of the last
    pass and converged (the last update ended on rematch_num >= 2).  The covariance is the reference's raw (I - K_1 G) P; the library
    stores its symmetric part, a difference of a few 1e-17 here - eleven orders below TOL_COV."""
    inv, eye, norm = np.linalg.inv, np.eye, np.linalg.norm
    st = st0.copy()
    its, searches = [], 0
    if prior is not None:
        O.StateView(st).cov[:6, :6] = prior
    for u in range(updates):
        prop = st.copy()
        P = O.StateView(st).cov[:6, :6].copy()
        search, rem, sel = True, 0, None
        for it in range(max_it):
            r = tree.iterate_once(scan, st, search=search, imu_en=False, selected=sel, threads=4)
            searches += int(search)
            sel = r["selected"]
            G, g, eff = unpack6(r["out91"])
            K1 = inv(G + inv(P))
            v = O.state_boxminus(prop, st)[:6]
            sol = K1 @ g + v - K1 @ G @ v
            d = np.zeros(24)
            d[:6] = sol
            st = O.state_boxplus(st, d)
            conv = norm(sol[:3]) * 57.3 < 0.01 and norm(sol[3:]) * 100 < 0.015
            search = False
            if conv or (rem == 0 and it == max_it - 2):
                search, rem = True, rem + 1
            if rem >= 2 or it == max_it - 1:
                O.StateView(st).cov[:6, :6] = (eye(6) - K1 @ G) @ P
                break
        its.append(it + 1)
    if info is not None:
        info.update(searches=searches, total_residual=psc.total_residual_np(r)[1], converged=rem >= 2)
    return st, its, eff


def all_poses(small_world):
    """The 24 poses of pose_score_cases.parity_poses, flat: [(R_LI, T_LI, R, p), ...] - 23 with the identity extrinsic, then the perturbed
    pose with its extrinsic."""
    out = []
    for r_li, t_li, R, p in psc.parity_poses(small_world):
        out += [(r_li, t_li, R[k], p[k]) for k in range(len(R))]
    assert len(out) == 24
    return out


def dense_prior(seed=11):
    """A dense SPD 6 x 6 prior: A A^T of a random A, scaled to 1e-4 on the rotation block's diagonal and 1e-2 on the position block's."""
    A = np.random.default_rng(seed).normal(size=(6, 6))
    M = A @ A.T
    d = np.sqrt(np.r_[np.full(3, 1e-4), np.full(3, 1e-2)] / np.diag(M))
    P = M * d[:, None] * d[None, :]
    return 0.5 * (P + P.T)


def pose_errors(O, st_ref, pose12):
    """(|dp|, |dtheta|) between a reference state and a record's pose."""
    v = O.StateView(st_ref)
    R = np.asarray(pose12[:9]).reshape(3, 3)
    return float(np.linalg.norm(v.pos_end - pose12[9:])), float(np.linalg.norm(O.log_so3(v.rot_end.T @ R)))
