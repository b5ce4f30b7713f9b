"""What the point-kinematics tests share: the points of a test, and the reference values formed in numpy from the oracle's per-body kinematics and geometric
Jacobians — pos = R r + p, vel = ω × pos + v, acc = α × pos + a + ω × vel, Jp = J_ang × pos + J_lin column by column (oracle.body_kinematics,
oracle.geometric_jacobian of path(world → body))."""
import numpy as np


def depths(flat):
    d = np.zeros(flat.n_bodies, dtype=int)
    for b in range(flat.n_bodies):
        d[b] = 0 if flat.parent[b] < 0 else d[flat.parent[b]] + 1
    return d


def pick_points(flat, seed=5):
    """P = 5: a leaf, a child of the world, a second point on that body, a point with r = 0 (on the last body), the deepest body."""
    rng = np.random.default_rng(seed)
    parent = np.asarray(flat.parent)
    leaves = [b for b in range(flat.n_bodies) if not (parent == b).any()]
    top = int(np.flatnonzero(parent < 0)[0])
    bodies = np.array([leaves[0], top, top, flat.n_bodies - 1, int(np.argmax(depths(flat)))], dtype=np.int32)
    r = rng.standard_normal((5, 3))
    r[3] = 0
    return bodies, r


def off_path(flat, bodies):
    """(P, nv) bool: velocity coordinate c belongs to no joint on path(world → bodies[k])."""
    nvj = np.diff(np.append(np.asarray(flat.v_offset), flat.nv))
    mask = np.ones((len(bodies), flat.nv), dtype=bool)
    for k, b in enumerate(bodies):
        b = int(b)
        while b >= 0:
            mask[k, flat.v_offset[b]:flat.v_offset[b] + nvj[b]] = False
            b = int(flat.parent[b])
    return mask


def reference(oracle, flat, q, v, vd, bodies, r, dtype=np.float64, jac=True):
    """(pos, vel, acc) as (B, P, 3) and Jp as (B, P, 3, nv) (None without `jac`); every operation in `dtype`."""
    B, P = q.shape[0], len(bodies)
    zero = np.zeros((B, flat.nv))
    H, T, A = oracle.body_kinematics(flat, q, zero if v is None else v, zero if vd is None else vd, dtype=dtype)
    r = np.asarray(r, dtype=dtype)
    pos, vel, acc = (np.zeros((B, P, 3), dtype) for _ in range(3))
    Jp = np.zeros((B, P, 3, flat.nv), dtype) if jac else None
    for k, b in enumerate(bodies):
        R, p = H[:, b, :9].reshape(B, 3, 3), H[:, b, 9:]
        pos[:, k] = np.einsum("bij,j->bi", R, r[k]) + p
        vel[:, k] = np.cross(T[:, b, :3], pos[:, k]) + T[:, b, 3:]
        acc[:, k] = np.cross(A[:, b, :3], pos[:, k]) + A[:, b, 3:] + np.cross(T[:, b, :3], vel[:, k])
        if jac:
            J, _ = oracle.geometric_jacobian(flat, q, -1, int(b), dtype=dtype)  # (B, 6, nv)
            for c in range(flat.nv):
                Jp[:, k, :, c] = np.cross(J[:, :3, c], pos[:, k]) + J[:, 3:, c]
    return pos, vel, acc, Jp


def pos_vel_fd(oracle, flat, q, v, bodies, r, dq, dv, h=1e-3):
    """The derivative of (pos, vel) along (dq, dv) per state by the 4-point central difference of the reference, in the raw coordinates q."""
    f = lambda s: np.concatenate([x.reshape(q.shape[0], -1) for x in reference(oracle, flat, q + s * h * dq, v + s * h * dv, None, bodies, r, jac=False)[:2]], axis=1)
    return (8 * (f(1) - f(-1)) - (f(2) - f(-2))) / (12 * h)
