"""CPU checks of the collision case generator (tests/collision_cases.py): the oracle's crash flags against a float64 sphere / box
distance that shares no formula with it (the collision oracle's arithmetic is "parity unpinned", oracle_dynamics.c), the share of
cases too close to the radius for float32 to decide, and the coverage each family promises."""
import numpy as np
import pytest

import collision_cases as cc


@pytest.fixture(scope="module")
def families(orc):
    return cc.cpu_families()


def test_float64_distance_is_the_definition():
    """hand-made cases of obb_distance64: inside, off a face, off an edge, off a corner of a box rotated by 90 degrees about z"""
    q = np.array([0.0, 0.0, np.sin(np.pi / 4), np.cos(np.pi / 4)])  # box x axis -> world y
    box = np.concatenate([[1.0, 2.0, 3.0], q, [0.5, 0.2, 0.1]])
    for p, want in (([1.0, 2.0, 3.0], 0.0), ([1.1, 2.4, 3.05], 0.0), ([1.0, 3.0, 3.0], 0.5), ([1.5, 2.0, 3.0], 0.3),
                    ([1.5, 2.9, 3.0], np.hypot(0.3, 0.4)), ([0.5, 1.1, 2.7], np.sqrt(0.3 ** 2 + 0.4 ** 2 + 0.2 ** 2))):
        assert abs(cc.obb_distance64(np.array(p), box) - want) < 1e-12, (p, want)


def test_oracle_flags_equal_the_float64_geometry(families, parity):
    """every family except grazing: oracle flag == (float64 distance < r) on all non-ambiguous envs, ambiguous <= 2 %; and per
    (sub-step, env) too, from the per-sub-step oracle queries"""
    for name, (state, action, boxes, expected, m) in families:
        amb = m["ambiguous"]
        parity.record(f"collision_cases/{name}/ambiguous share", amb.mean(), None if m["family"] == "grazing" else 0.02, "fraction")
        parity.record(f"collision_cases/{name}/hit share", expected.mean(), None, "fraction")
        if m["family"] == "grazing":
            continue
        assert amb.mean() <= 0.02, (name, amb.mean())
        assert np.array_equal(expected[~amb], m["flags64"][~amb]), (name, np.nonzero(expected != m["flags64"])[0])
        per_substep64 = (m["d64"] < m["r"]).any(-1)
        assert np.array_equal(m["hits_per_substep"][:, ~amb], per_substep64[:, ~amb]), name


def test_grazing_is_what_float64_cannot_decide(families, parity):
    """the grazing cases sit within r 2^-16 of the radius: both outcomes occur (asserted by the generator), and float64 agrees with
    the oracle wherever the separation is outside the float32 error bound"""
    for name in ("grazing", "grazing[quad_no_control]"):
        state, action, boxes, expected, m = dict(families)[name]
        amb = m["ambiguous"]
        assert 0.25 <= expected.mean() <= 0.75, name
        assert np.array_equal(expected[~amb], m["flags64"][~amb]), name
        i = np.arange(expected.size)
        rel = np.abs(m["d64"][:, i, i % boxes.shape[1]].min(0) / m["r"] - 1.0)
        assert rel.max() < 2.0 ** -15 and (rel > 2.0 ** -21).mean() > 0.8, name  # the placement is where it was meant to be


def test_count_edges_coverage(families, parity):
    for name, (state, action, boxes, expected, m) in families:
        if m["family"] != "count_edges":
            continue
        n, K = boxes.shape[:2]
        hi = m["hit_index"]
        seen = set(hi[hi >= 0].tolist())
        classes = cc.hit_index_classes(K)
        assert set(classes.values()) <= seen, (name, {c: i for c, i in classes.items() if i not in seen})
        parity.record(f"collision_cases/{name}/hit-index classes seen", len(classes), None, "count")
        assert np.array_equal(expected, hi >= 0), name  # exactly the envs meant to crash
        assert np.array_equal(np.arange(n) % 3 == 1, hi < 0)  # a third without a hit, interleaved
        # exactly ONE box hits, the one at the chosen index
        hits = (m["d64"] < m["r"]).any(0)
        assert np.array_equal(hits.sum(-1), (hi >= 0).astype(int)) and hits[hi >= 0, hi[hi >= 0]].all(), name
        # every box that is not parked gets past the cull, so the predicate runs on it; the parked ones do not
        assert m["passes_cull"][~m["parked"]].all() and not m["passes_cull"][m["parked"]].any(), name
        assert m["parked"].sum(-1).tolist() == [2 if K >= 8 else 0] * n


def test_substep_only_coverage(families):
    for name, (state, action, boxes, expected, m) in families:
        if m["family"] != "substep_only":
            continue
        k, n = m["k"], expected.size
        assert n == 2 * k + 3 and expected.all()
        assert set(m["hit_substep"].tolist()) == set(range(k)), name  # every s, first and last included
        hps = m["hits_per_substep"]
        assert np.array_equal(hps, np.arange(k)[:, None] == m["hit_substep"][None, :]), name  # hit at s and at no other sub-step
        # consecutive positions are further apart than 0.2 r
        step = np.linalg.norm(np.diff(m["traj"].astype(np.float64), axis=0), axis=-1)
        assert step.min() > 0.2 * m["r"], (name, step.min() / m["r"])


def test_cull_adversaries_coverage(families):
    for name in ("cull_adversaries", "cull_adversaries[quad_no_control]"):
        _adversary_pairs(*dict(families)[name])


def _adversary_pairs(state, action, boxes, expected, m):
    assert np.array_equal(expected, m["wants_hit"])  # each pair: once a hit, once a near miss
    assert expected[0::2].all() and not expected[1::2].any()
    kinds = set(m["pair_kind"])
    assert kinds == {"beam_tip", "slab_above", "slab_below", "robot_at_centre", "deep_inside", "fast_through"}
    n, K = boxes.shape[:2]
    adv = boxes[np.arange(n), np.arange(n) % K]
    far = np.linalg.norm(adv[:, 0:3].astype(np.float64) - m["traj"][-1], axis=-1)
    is_beam = np.repeat(np.array(m["pair_kind"]) == "beam_tip", 2)
    assert (far[is_beam] > 3.9).all()  # the touched beam's centre is 4 m away
    assert (m["traj"][-1] != m["final_state"][:, 0:3]).sum() == 0
    # the final position alone (the stand-alone entry point) sees hits and misses as well
    last = m["hits_per_substep"][-1]
    assert last.any() and (expected & ~last).any()
