"""Test helper: numpy-float32 restatement of the two places where the env step of a multirotor whose centre of mass is off the
base-link origin (agx_env_step_com, DESIGN.md "integrator") differs from the ordinary one -- the lever arm of the root body's force
and the base-link position behind the integrator -- on top of the oracle for everything the two share.  It is the comparator of
the GPU tests; tests/test_com_offset.py checks that it conserves what it must and that c = 0 is the oracle's step.

Every array is float32 and every + - * one rounded float32 operation; the fused multiply-subtract inside torch.cross is explicit
(sim2real_ref.cross, the kernels' `cross`)."""
import numpy as np
from sim2real_ref import cross, f32, norm3, quat_rotate

F = np.float32


def com_of(pd):
    """the composite's centre of mass in the base-link frame, fp32 [3] (robot_params_dict's `com`; absent: the origin)"""
    return f32(pd.get("com", [0.0, 0.0, 0.0]))


def lever_torque(f_root, c):
    """torque about the mass centre of the force f_root [N, 3] acting at the base-link origin, -c from it: (-c) x f = f x c"""
    f_root = f32(f_root)
    return cross(f_root, np.broadcast_to(f32(c), f_root.shape))


def correct_position(p, q0, q1, c):
    """the base-link origin behind integrate(): p holds p + v dt, the body turned from q0 to q1 about its mass centre"""
    cc = np.broadcast_to(f32(c), f32(p).shape)
    return f32(p) + (quat_rotate(f32(q0), cc) - quat_rotate(f32(q1), cc))


def root_force(vbody, pd, disturb=None, disturb_max=None):
    """force of the root body's entry of robot_force_tensor with the allocator's forces at the motor links: 0, `+=` the drag
    (base_multirotor.py:260-285: -c_l[k] v[k] - c_q[k] |v| v[k]), `+=` the disturbance (:213-234; disturb [N, 7] = occurrence |
    six uniforms).  An absent term is +0."""
    v = f32(vbody)
    lin, quad = f32(pd["lin_drag_linear"])[None, :], f32(pd["lin_drag_quadratic"])[None, :]
    f = ((-lin) * v) + (((-quad) * norm3(v)[:, None]) * v)
    if disturb is None:
        return f + F(0.0)
    d, m = f32(disturb), f32(disturb_max)[None, 0:3]
    return f + (((m - (-m)) * d[:, 1:4] + (-m)) * d[:, 0:1])


def substep(orc, P, pd, state, action, thrust, kT, tau_inc, tau_dec, Kp, Kv, KR, Kw, disturb=None, disturb_max=None, com=None):
    """one physics sub-step in place on `state` [N, 13] and `thrust` [N, M] -> the oracle's SubstepOut (derived tensors of the
    pre-physics state, wrench command; body_wrench with the lever arm added).  com None: pd's."""
    c = com_of(pd) if com is None else f32(com)
    q0 = state[:, 3:7].copy()
    o = orc.substep(P, state, action, thrust, kT, tau_inc, tau_dec, Kp, Kv, KR, Kw, disturb=disturb, disturb_max=disturb_max, integrate=False)
    bw = o.body_wrench
    f_root = bw[:, 0:3] if int(pd.get("root_link_mode", 0)) else root_force(o.vbody, pd, disturb, disturb_max)
    bw[:, 3:6] = bw[:, 3:6] + lever_torque(f_root, c)
    orc.integrate(P, state, np.ascontiguousarray(bw))
    state[:, 0:3] = correct_position(state[:, 0:3], q0, state[:, 3:7], c)
    return o


def body_wrench_substep(orc, P, state, body_wrench, com):
    """the integrating launch of the plug-in path (AGX_LAUNCH_BODY_WRENCH): the net wrench about the mass centre as handed in"""
    q0 = state[:, 3:7].copy()
    orc.integrate(P, state, np.ascontiguousarray(f32(body_wrench)))
    state[:, 0:3] = correct_position(state[:, 0:3], q0, state[:, 3:7], com)
