"""Test helper: the edge fixtures tests/golden/step_edge_<robot>_<ctrl>.npz (oracle/gen_golden.py, EdgeSource) -- the reference's
BaseMultirotor.step on every attitude (the special rows of get_euler_xyz / atan2 / the angle wraps, then the whole sphere),
velocities at rest / nominal / beyond the clamps, motor thrusts at their limits, at zero and negative, actions at zero / nominal /
beyond the clips, and command rows for the controllers' special cases -- and the gate every implementation is held to on them."""
import numpy as np
from conftest import elem_err, err_where_reference_is_defined, max_abs

BASE_CASES = ["quad_position", "quad_velocity", "quad_attitude", "quad_acceleration", "quad_no_control",
              "octarotor_position", "octarotor_velocity", "octarotor_fully_actuated", "quad_rates", "quad_velocity_steering"]
EDGE_CASES = ["edge_" + c for c in BASE_CASES]  # load_golden("step_" + case)
TOL = 1e-5
# at most this share of the elements of any array may fall under the "reference undefined" exemption of
# conftest.err_where_reference_is_defined (the reference's own result moves by more than half the gate with its math library)
UNDEFINED_CAP = 0.01
FIXED_ROWS = 24  # the table's first rows are the fixed special attitudes


def angle_err(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return float(np.minimum(d, 2 * np.pi - d).max())


def gates_vs_reference(parity, tag, case, g, k, got, full_scale_thrust):
    """One recorded sub-step `k` of an edge fixture `g` against what an implementation returned on its inputs (`got`: euler, qveh,
    vveh, vbody, wbody, wrench, thrust, next_state): |err| <= 1e-5 max(1, |x|) per element (thrusts: of the full-scale thrust),
    over the elements where the reference's own answer is defined to that gate wherever the generator recorded the correctly
    rounded twin (`*_cr`), the correctly rounded answer exactly elsewhere -- and at most UNDEFINED_CAP of any array elsewhere."""
    K = g["state"].shape[0]

    def where_defined(name, x, ref, ref_cr, scale=1.0):
        x, ref, ref_cr = (np.asarray(a, np.float64) / scale for a in (x, ref, ref_cr))
        worst, n_undef, exact_there = err_where_reference_is_defined(x, ref, ref_cr, TOL)
        parity.record(f"{tag}_{name}_vs_reference[{case}] [abs, all elements]", max_abs(x, ref), None, "abs")
        parity.record(f"{tag}_{name}_vs_reference[{case}] [elements where the reference's own libm spread > gate / 2]", n_undef, None, "count")
        parity.check(f"{tag}_{name}_vs_reference[{case}]", worst, TOL, "|err| / max(1, |x|)", k)
        assert exact_there, (case, k, name, "not the correctly rounded answer where the reference is ill-conditioned")
        assert n_undef <= UNDEFINED_CAP * x.size, (case, k, name, n_undef, x.size)

    parity.check(f"{tag}_euler_vs_reference[{case}]", angle_err(got["euler"], g["euler"][k]), TOL, "rad", k)
    for name in ("qveh", "vveh", "vbody"):
        parity.check(f"{tag}_{name}_vs_reference[{case}]", elem_err(got[name], g[name][k]), TOL, "|err| / max(1, |x|)", k)
    where_defined("wbody", got["wbody"], g["wbody"][k], g["wbody_cr"][k])
    where_defined("thrust", got["thrust"], g["thrust_out"][k], g["thrust_out_cr"][k], full_scale_thrust)
    if "no_control" not in case:
        where_defined("wrench", got["wrench"], g["wrench_cmd"][k], g["wrench_cmd_cr"][k])
    if k + 1 < K:  # the generator advanced the reference's wrench with the oracle integrator: state[k + 1]
        for name, sl in (("position", slice(0, 3)), ("quaternion", slice(3, 7)), ("linvel", slice(7, 10)), ("angvel", slice(10, 13))):
            where_defined(f"next_state/{name}", got["next_state"][:, sl], g["state"][k + 1][:, sl], g["state_next_cr"][k][:, sl])


def arrangement(n, rotate=0, cut=None):
    """env order of a run: position p of the batch holds env (p + rotate) % n of the table; `cut` keeps the first `cut` positions"""
    idx = (np.arange(n) + rotate) % n
    return idx if cut is None else idx[:cut]
