"""The float64 reference of the capsule proximity (tests/proximity_ref.py) pinned
without a GPU: against a dense, refined brute force over (s, t) on random
segments, against known answers (two spheres, crossed perpendicular axes,
end point to end point, end point to interior, exactly parallel axes
overlapping and not, collinear axes, both axes degenerate), under swapping a
pair and under a rigid motion.  Then, from the reference alone: the GPU test's
scenarios keep the exclusion caps (2 % of a case's pairs for dist, 5 % for the
witness positions), their crossed-leg env penetrates, and the walk's default
capsule set is clear of the default margin at the default stance.  The Python
helpers that build capsules and pairs from the link tree are checked here too."""
import os

import numpy as np
import pytest

from tests import proximity_ref as pr

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_segments(rs, n):
    for k in range(n):
        p = rs.uniform(-1.0, 1.0, (4, 3))
        if k % 5 == 1:
            p[3] = p[2] + (p[1] - p[0]) * rs.uniform(0.3, 2.0)            # parallel
        if k % 5 == 2:
            p[1] = p[0]                                                   # a point
        if k % 5 == 3:
            p[3] = p[2] + (p[1] - p[0]) + rs.normal(0, 1e-4, 3)           # nearly parallel
        yield p


def test_reference_matches_a_refined_brute_force_on_random_segments():
    rs = np.random.default_rng(5)
    worst = 0.0
    for p in _random_segments(rs, 60):
        delta, s, t = pr.segments(*p)
        assert 0.0 <= s <= 1.0 and 0.0 <= t <= 1.0
        w = (p[0] + s * (p[1] - p[0])) - (p[2] + t * (p[3] - p[2]))
        assert abs(np.linalg.norm(w) - delta) <= 1e-12                    # the minimiser attains the distance
        b = pr.brute(*p)
        assert delta <= b + 1e-12                                         # no grid point is closer
        worst = max(worst, b - delta)
    assert worst <= 1e-6                                                  # (the brute force's own resolution)


@pytest.mark.parametrize("name,a,b,delta", pr.KNOWN, ids=[k[0] for k in pr.KNOWN])
def test_known_answers(name, a, b, delta):
    got, s, t = pr.segments(a[0], a[1], b[0], b[1])
    assert abs(got - delta) <= 1e-12, (name, got, delta)
    again, t2, s2 = pr.segments(b[0], b[1], a[0], a[1])                   # the pair swapped
    assert abs(again - got) <= 1e-15


def test_known_set_covers_the_degenerate_cases():
    names = [k[0] for k in pr.KNOWN]
    for want in ("two spheres", "crossed perpendicular", "end to end", "end to interior", "parallel overlapping",
                 "parallel apart", "collinear apart", "collinear overlapping", "both degenerate"):
        assert want in names
    caps, pairs, want = pr.known_capsules()
    assert len(caps) == 32 and len(pairs) == 16 and want.shape == (16,)


def test_swapping_a_pair_swaps_the_witness_and_keeps_the_rest():
    rs = np.random.default_rng(6)
    p0, p1 = rs.uniform(-1, 1, (6, 3)), rs.uniform(-1, 1, (6, 3))
    rad = rs.uniform(0.01, 0.1, 6)
    pairs = [(0, 1), (2, 3), (4, 5), (0, 5), (1, 4)]
    d, w, s, *_ = pr.proximity_points(p0, p1, rad, pairs, 0.3)
    d2, w2, s2, *_ = pr.proximity_points(p0, p1, rad, [(b, a) for a, b in pairs], 0.3)
    assert np.allclose(d, d2, atol=1e-15) and np.allclose(s, s2, atol=1e-13)
    assert np.allclose(w[:, :3], w2[:, 3:], atol=1e-12) and np.allclose(w[:, 3:], w2[:, :3], atol=1e-12)
    assert s[2] == (d < 0.3).sum() and abs(s[3] - np.maximum(0.3 - d, 0).sum()) < 1e-15 and s[1] == np.argmin(d)


def test_a_rigid_motion_of_the_root_moves_the_witness_and_nothing_else():
    m, caps, pairs, root, dof = pr.scenario("thormang")
    ref = pr.reference("thormang")
    # env 1 is env 0 moved by FAR
    assert np.allclose(ref.dist[0], ref.dist[1], atol=1e-12) and np.allclose(ref.summary[0], ref.summary[1], atol=1e-10)
    shift = root[1, :3].astype(np.float64) - root[0, :3].astype(np.float64)
    assert np.allclose(ref.witness[1] - ref.witness[0], np.tile(shift, 2), atol=1e-12)
    # a turned root: the same distances
    turned = root[:1].copy()
    c, s = np.cos(0.7), np.sin(0.7)
    q = turned[0, 3:7].astype(np.float64)
    turned[0, 3:7] = pr._quat_mul(np.array([0.0, 0.0, s, c]), q)
    D = m.num_dof
    other = pr.proximity_ref(m, turned, dof[:D], list(caps), list(pairs), pr.MARGIN)
    assert np.abs(other.dist[0] - ref.dist[0]).max() <= 1e-6              # (fp32 quaternion of the turned root)


@pytest.mark.parametrize("case", pr.CASES)
def test_scenarios_keep_the_exclusion_caps(case):
    for n, seed in ((pr.N, 12), (1, 13)):
        m, caps, pairs, root, dof = pr.scenario(case, n, seed)
        ref = pr.reference(case, n, seed)
        assert ref.dist.shape == (n, len(pairs)) and np.isfinite(ref.dist).all()
        if case == "kat_free":
            continue                                                      # known answers: compared on dist alone
        assert 1.0 - ref.keep_dist.mean() <= pr.DIST_CAP, case
        assert 1.0 - ref.keep_witness.mean() <= pr.WITNESS_CAP, case
        assert len(caps) <= 32 and 1 <= len(pairs) <= 256


def test_thormang_scenario_has_a_crossed_leg_env_and_a_far_twin():
    m, caps, pairs, root, dof = pr.scenario("thormang")
    ref = pr.reference("thormang")
    assert (ref.dist[pr.CROSSED_ENV] < 0).sum() >= 3 and ref.summary[pr.CROSSED_ENV, 2] >= 3
    assert np.hypot(*(root[1, :2] - root[0, :2])) > 30.0 and np.array_equal(root[1, 3:], root[0, 3:])
    assert (np.abs(dof[:, 0]) <= 0.6).all()


def _walk_cfg():
    import yaml
    with open(os.path.join(REPO, "thormang_isaacgym_amd", "cfg", "task", "ThormangWalk.yaml")) as f:
        return yaml.safe_load(f)


@pytest.mark.parametrize("model", ["thormang", "thormang_wb"])
def test_walks_default_set_is_clear_of_the_margin_at_the_default_stance(model):
    from thormang_isaacgym_amd.sim import capsule_pairs, link_tree, load_model
    from thormang_isaacgym_amd.tasks.thormang_walk import WALK_SELF_MARGIN, walk_self_capsules
    m = load_model(model)
    caps = walk_self_capsules(m)
    pairs = capsule_pairs(link_tree(m)[0], caps)
    assert len(caps) == 15 and len(pairs) == 99
    cfg = _walk_cfg()
    assert "enableSelfProximity" not in cfg["env"] and "selfProximityMargin" not in cfg["env"]
    root, dof = pr.default_stance(m, cfg["env"]["defaultJointAngles"])
    ref = pr.proximity_ref(m, root, dof, pr.capsule_tuples(caps), pairs, WALK_SELF_MARGIN)
    assert WALK_SELF_MARGIN == 0.02
    assert ref.dist.min() >= WALK_SELF_MARGIN + 0.005, ref.dist.min()
    assert ref.summary[0, 2] == 0 and ref.summary[0, 3] == 0.0
    assert all(0.0299 <= c.radius <= 0.0901 for c in caps)


def test_limb_capsules_follow_the_link_tree():
    from thormang_isaacgym_amd.sim import limb_capsule, link_tree, load_model
    m = load_model("thormang")
    parent, origin = link_tree(m)
    li = m.link_index
    thigh = limb_capsule(parent, origin, li("l_leg_hip_p_link"), li("l_leg_kn_p_link"), 0.06)
    assert thigh.link == li("l_leg_hip_p_link") and list(thigh.p0) == [0.0, 0.0, 0.0]
    assert np.allclose(list(thigh.p1), [0.0, 0.06, -0.3], atol=1e-7) and abs(thigh.radius - 0.06) < 1e-8
    for link, child in (("l_leg_kn_p_link", "l_leg_an_p_link"), ("r_arm_sh_p2_link", "r_arm_el_y_link"),
                        ("r_arm_el_y_link", "r_arm_wr_r_link")):
        c = limb_capsule(parent, origin, li(link), li(child), 0.05)
        assert np.linalg.norm(list(c.p1)) > 0.15
    with pytest.raises(ValueError):
        limb_capsule(parent, origin, li("l_leg_hip_p_link"), li("l_leg_an_p_link"), 0.05)   # a grandchild


def test_capsule_pairs_leave_out_neighbours_and_are_bounded():
    from thormang_isaacgym_amd.sim import capsule_pairs, link_hops, link_tree, load_model, make_capsule
    m = load_model("thormang")
    parent, _origin = link_tree(m)
    li = m.link_index
    links = ["pelvis_link", "pelvis_link", "chest_link", "head_y_link", "l_leg_hip_y_link", "l_leg_hip_r_link",
             "l_leg_hip_p_link", "r_leg_hip_y_link"]
    caps = [make_capsule(li(n), (0, 0, 0), None, 0.01) for n in links]
    assert link_hops(parent, li("l_leg_hip_p_link"), li("pelvis_link")) == 3
    assert link_hops(parent, li("l_leg_hip_y_link"), li("r_leg_hip_y_link")) == 2
    assert link_hops(parent, li("l_leg_foot_link"), li("r_arm_end_link")) == 7 + 9
    pairs = capsule_pairs(parent, caps)
    for a, b in pairs:
        assert a < b and link_hops(parent, caps[a].link, caps[b].link) >= 3
    assert (0, 1) not in pairs and (0, 2) not in pairs and (0, 3) not in pairs and (0, 4) not in pairs
    assert (0, 6) in pairs and (1, 6) in pairs and (2, 6) in pairs and (4, 7) not in pairs and (5, 7) in pairs
    assert pairs == sorted(pairs)
    assert (0, 1) in capsule_pairs(parent, caps, min_hops=0) and len(capsule_pairs(parent, caps, min_hops=0)) == 28
    many = [make_capsule(li("pelvis_link") if k % 2 else li("l_leg_foot_link"), (0, 0, 0), None, 0.01)
            for k in range(32)]
    assert len(capsule_pairs(parent, many)) == 256
    many.append(make_capsule(li("r_leg_foot_link"), (0, 0, 0), None, 0.01))
    with pytest.raises(ValueError):
        capsule_pairs(parent, many)
