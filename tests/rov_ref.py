"""Test helper: numpy-float32 restatement of the three places where the reference's BaseROV (robots/base_rov.py) differs from
BaseMultirotor -- the drag, the Euler angles, the reset -- on top of what the other helpers provide (sim2real_ref: the Euler
conversions; the oracle: everything the two robot kinds share).  It is the comparator of the GPU tests (the reference's code does
not exist where they run) and is itself pinned to the reference bit for bit by tests/test_base_rov.py (tests/golden/rov_cr/*.npz:
the reference's own code with correctly rounded elementary functions).

Every array is float32 and every + - * one rounded float32 operation; sin / cos / atan2 / asin are evaluated in float64 and rounded
once (sim2real_ref._el)."""
import os

import numpy as np
from sim2real_ref import euler_xyz, f32, quat_from_euler_xyz

F = np.float32
DERIVED = ("euler", "qveh", "vveh", "vbody", "wbody")  # the five derived tensors, in the order of the device's derived block
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_golden(name, cr=False):
    """cr=True: the fixture made by the reference's code with correctly rounded elementary functions (tests/golden/rov_cr/)"""
    return np.load(os.path.join(GOLDEN, *(["rov_cr"] if cr else []), name + ".npz"))


def same(a, b):
    """bit for bit, as this suite reads it everywhere: same shape, every element equal (np.array_equal: a zero equals a zero of
    either sign -- the vehicle-frame quaternion's x component is -0 in torch and +0 in the kernels' quat_from_yaw)"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(np.array_equal(a, b))


def disturb_of(g, k):
    """the host-supplied disturbance draws of sub-step k of a step fixture ([N, 7]), None where the record has none"""
    return g["disturb"][k] if g["disturb"][k].any() else None


def euler(q):
    """update_states (base_rov.py:251-252): get_euler_xyz_tensor(q) as it is -- angles in [0, 2 pi), no ssa()"""
    return euler_xyz(f32(q))


def drag(vbody, wbody, pd):
    """simulate_drag (base_rov.py:260-285) -> (force [N, 3], torque [N, 3]) added to the root body: linear + quadratic term, the
    quadratic one PER AXIS for the linear velocity too (-c_q[k] |v[k]| v[k]; the multirotor's is -c_q[k] |v| v[k])"""
    out = []
    for x, lin, quad in ((f32(vbody), pd["lin_drag_linear"], pd["lin_drag_quadratic"]), (f32(wbody), pd["ang_drag_linear"], pd["ang_drag_quadratic"])):
        lin, quad = f32(lin)[None, :], f32(quad)[None, :]
        out.append(((-lin) * x) + (((-quad) * np.abs(x)) * x))
    return out[0], out[1]


def root_wrench(vbody, wbody, pd, disturb=None, disturb_max=None):
    """row 0 of robot_force_tensor / robot_torque_tensor as BaseROV.step leaves it with the forces at the motor links: 0, `+=` the
    drag, `+=` the disturbance (disturb: [N, 7] = occurrence | six uniforms, apply_disturbance base_rov.py:206-227)"""
    f, t = drag(vbody, wbody, pd)
    f, t = F(0.0) + f, F(0.0) + t
    if disturb is not None:
        d, m = f32(disturb), f32(disturb_max)[None, :]
        w = ((m - (-m)) * d[:, 1:7] + (-m)) * d[:, 0:1]
        f, t = f + w[:, 0:3], t + w[:, 3:6]
    return f, t


def reset(mask, state, u_state, min_state, max_state, bounds_min, bounds_max):
    """reset_idx (base_rov.py:171-198) -> the new state tensor: the envs of `mask` respawn from the [N, 13] uniform draw, nobody
    else moves; the motor model is not touched at all (no draws, thrusts and constants stay)"""
    mask = np.asarray(mask).astype(bool)
    lo, hi = f32(min_state)[None, :], f32(max_state)[None, :]
    r = (hi - lo) * f32(u_state) + lo
    bmin, bmax = np.broadcast_to(f32(bounds_min), (len(mask), 3)), np.broadcast_to(f32(bounds_max), (len(mask), 3))
    new = f32(state).copy()
    pos = bmin + (bmax - bmin) * r[:, 0:3]
    new[mask, 0:3] = pos[mask]
    new[mask, 3:7] = quat_from_euler_xyz(r[:, 3:6])[mask]
    new[mask, 7:13] = r[mask, 7:13]
    return new


def reset_gains(mask, gains, u_gains, gains_min, gains_max):
    """the controller's randomize_params(env_ids) that ends reset_idx (base_lee_controller.py:101-118)"""
    mask = np.asarray(mask).astype(bool)
    lo, hi = f32(gains_min)[None, :], f32(gains_max)[None, :]
    new = f32(gains).copy()
    new[mask] = ((hi - lo) * f32(u_gains) + lo)[mask]
    return new
