"""The capsule proximity on the GPU (tg_proximity, Sim.proximity) against the
float64 reference (tests/proximity_ref.py, pinned by
tests/test_proximity_reference.py), which also builds the scenarios.

Sims of five envs and of one: random headings, tilts of 0.05 .. 0.15 rad and
joint angles within +-0.4 rad.  Env 1 has env 0's pose 50 m away: its dist and
summary must have env 0's bits, its witness env 0's shifted.  On thormang env 2
stands with crossed legs, so several pairs penetrate.  Models: thormang with the
walk's default capsules and Sim.capsule_pairs (15 capsules, 99 pairs); gogoro
with the rider's forearms and hands against capsules on the scooter's head and
body links; jit_walker, compiled at run time; kat_free, one link carrying the
32 capsules of the known answers (every distance a constant, the degenerate
configurations among them).  Every output is filled with NaN before each call.

Exact checks, no tolerance: summary[0] has the bits of the smallest element of
the GPU's own dist row, summary[1] is its first index, summary[2] the count of
dist < margin in that row.  The witness points lie on their segments and their
separation is dist + r_a + r_b, both to the witness tolerance below.

Exclusions (proximity_ref's conditions).  A pair whose reference axis distance
is under AXIS_MIN = 5 mm leaves the dist comparison and must read a finite
value of at most AXIS_MIN - r_a - r_b plus the tolerance; at most 2 % of a
case's pairs.  A pair whose unclamped Hessian is nearly singular leaves the
witness-position comparison; at most 5 %.  kat_free's known answers are compared
on dist alone.  summary[1] is compared where the reference's two smallest
distances differ by more than twice the tolerance, summary[2] where no pair
lies within the tolerance of the margin.

Tolerance.  Measured per case on the MI355X on this file's first run
(PROX_MEASURED below; the worst over every comparison the file makes for the
case): max |got - ref| of dist and of witness in metres, of summary[0], and of
summary[3] / P.  Asserted: 4 x the measured value, under the project's hard cap
of 1e-4.  Worst measured: dist 2.3e-7 m (thormang), the rounding of
root-relative coordinates of about 1 m; witness 1.95e-6 m, half an fp32 ulp of
a world coordinate of 30 .. 70 m, which the root position added last brings in
(1.9e-6 is exactly what env 1's witness differs by from env 0's shifted);
summary[0] 1.4e-7 m; summary[3] / P 1.7e-8 m.  At most 0.2 % of a comparison's
pairs were left out of dist and 1.0 % out of the witness positions."""
import numpy as np
import pytest
import torch

from tests import physics_models as pm
from tests import proximity_ref as pr
from thormang_isaacgym_amd import abi

pytestmark = pytest.mark.gpu

N = pr.N
MARGIN = pr.MARGIN
# max |got - ref| of dist, witness (m), summary[0] (m) and summary[3] / P (m), measured on the MI355X: the worst over
# every comparison this file makes for the case
PROX_MEASURED = {
    #              dist    witness  summary0  summary3 / P
    "thormang":    [2.3e-7, 1.91e-6, 1.37e-7, 1.72e-8],
    "gogoro":      [2.26e-7, 1.95e-6, 1.12e-7, 4.6e-10],
    "jit_walker":  [4.5e-8, 1.73e-6, 6.2e-9, 0.0],       # (no pair near the margin: the penalty is 0 on both sides)
    "kat_free":    [6.4e-8, 1.86e-6, None, None],        # (the smallest pair is an excluded one: no summary compared)
    "walk_task":   [None, None, 6.2e-8, 0.0],            # (the task test compares the summary; no pair under the margin)
}
HARD_CAP = 1e-4
assert all(4 * v <= HARD_CAP for row in PROX_MEASURED.values() for v in row if v is not None)
OUTPUTS = ("dist", "witness", "summary0", "summary3")


def tolerance(case, output):
    """4 x the measured value; 0 where the table has None: nothing is compared there, and check's figure is 0."""
    return 4 * (dict(zip(OUTPUTS, PROX_MEASURED[case]))[output] or 0.0)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device="cuda:0")


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Case:
    """A sim of ``n`` envs in the scenario's state."""

    def __init__(self, case, n=N, seed=12):
        if not torch.cuda.is_available():
            pytest.skip("needs the MI355X")
        from thormang_isaacgym_amd.sim import Sim
        self.case, self.n, self.seed = case, n, seed
        self.m, caps, pairs, self.root, self.dof = pr.scenario(case, n, seed)
        self.caps, self.pairs = list(caps), list(pairs)
        m = self.m
        self.s = s = Sim(m, pm.sim(m, n=n, dt=0.01, substeps=1)[1], n, "cuda:0")
        s.root_state.copy_(torch.from_numpy(self.root))
        s.dof_state.copy_(torch.from_numpy(self.dof))
        s.refresh()
        self.ref_state = (self.root, self.dof)        # the state the references passed to check are made of

    def call(self, caps=None, pairs=None, margin=MARGIN, want=("dist", "witness", "summary")):
        """One call of the C function on NaN-filled outputs; (dist, witness, summary) as numpy, NaN where not asked."""
        from thormang_isaacgym_amd._lib import lib
        caps = self.caps if caps is None else caps
        pairs = self.pairs if pairs is None else pairs
        P = len(pairs)
        d, w, sm = _nan(self.n, P), _nan(self.n, P, 6), _nan(self.n, 4)
        arr = (abi.tg_capsule * len(caps))(*pr.as_structs(caps))
        idx = (abi.C.c_int32 * (2 * P))(*[int(v) for ab in pairs for v in ab])
        pp = abi.tg_proximity_params()
        pp.margin = margin
        rc = lib().tg_proximity(self.s.handle, arr, len(caps), idx, P, pp,
                                d.data_ptr() if "dist" in want else None,
                                w.data_ptr() if "witness" in want else None,
                                sm.data_ptr() if "summary" in want else None)
        assert rc == 0, lib().tg_last_error()
        torch.cuda.synchronize()
        return d.cpu().numpy(), w.cpu().numpy(), sm.cpu().numpy()

    def reference(self, caps=None, pairs=None, margin=MARGIN, root=None, dof=None):
        if caps is None and pairs is None and root is None and margin == MARGIN:
            return pr.reference(self.case, self.n, self.seed)
        return pr.proximity_ref(self.m, self.root if root is None else root, self.dof if dof is None else dof,
                                self.caps if caps is None else caps, self.pairs if pairs is None else pairs, margin)

    def check(self, key, got, ref, caps=None, pairs=None, margin=MARGIN, case=None, quota=True):
        """The exact checks on one call and its comparison with the reference; prints and returns the figures."""
        case = case or self.case
        caps = self.caps if caps is None else caps
        pairs = self.pairs if pairs is None else pairs
        d, w, sm = got
        P = len(pairs)
        assert d.dtype == np.float32 and d.shape == (self.n, P) and w.shape == (self.n, P, 6) and sm.shape == (self.n, 4)
        assert np.isfinite(d).all() and np.isfinite(w).all() and np.isfinite(sm).all()        # every element written
        tol_d, tol_w = tolerance(case, "dist"), tolerance(case, "witness")
        ra = np.array([np.float32(caps[a][3]) for a, _b in pairs], np.float64)
        rb = np.array([np.float32(caps[b][3]) for _a, b in pairs], np.float64)
        # exact: the summary is that of the GPU's own dist row
        first = d.argmin(axis=1)
        assert np.array_equal(_bits(sm[:, 0]), _bits(d[np.arange(self.n), first])), key
        assert np.array_equal(sm[:, 1], first.astype(np.float32)), key
        assert np.array_equal(sm[:, 2], (d < np.float32(margin)).sum(axis=1).astype(np.float32)), key
        # the witness points lie on their segments (the reference's axes) and are dist + r_a + r_b apart
        wd = w.astype(np.float64)
        sep = np.linalg.norm(wd[..., :3] - wd[..., 3:], axis=-1)
        fig = {"separation": float(np.abs(sep - (d.astype(np.float64) + ra + rb)).max())}
        on = 0.0
        ends = self._ends(ref, caps)
        for e in range(self.n):
            for k, (a, b) in enumerate(pairs):
                for pt, c in ((wd[e, k, :3], a), (wd[e, k, 3:], b)):
                    on = max(on, np.sqrt(pr.point_segment(pt, ends[0][e, c], ends[1][e, c] - ends[0][e, c])[0]))
        fig["off_segment"] = float(on)
        # against the reference
        kd, kw = ref.keep_dist, ref.keep_witness
        fig["dist"] = float(np.abs(d - ref.dist)[kd].max(initial=0.0))
        fig["witness"] = float(np.abs(wd - ref.witness)[kw].max(initial=0.0))
        fig["excluded"], fig["excluded_witness"] = float(1.0 - kd.mean()), float(1.0 - kw.mean())
        min_kept = kd[np.arange(self.n), ref.summary[:, 1].astype(int)]
        fig["summary0"] = float(np.abs(sm[:, 0] - ref.summary[:, 0])[min_kept].max(initial=0.0))
        all_kept = kd.all(axis=1)
        fig["summary3"] = float(np.abs(sm[:, 3] - ref.summary[:, 3])[all_kept].max(initial=0.0)) / P
        print({"case": self.case, "n": self.n, "call": key, "P": P, **fig})
        if quota:
            assert fig["excluded"] <= pr.DIST_CAP and fig["excluded_witness"] <= pr.WITNESS_CAP, (key, fig)
        bound = pr.AXIS_MIN - ra - rb + tol_d
        assert (d[~kd] <= np.broadcast_to(bound, d.shape)[~kd]).all(), key
        assert fig["dist"] <= tol_d, (key, fig)
        assert fig["witness"] <= tol_w, (key, fig)
        assert fig["off_segment"] <= tol_w, (key, fig)
        assert fig["separation"] <= tol_w, (key, fig)
        assert fig["summary0"] <= tolerance(case, "summary0"), (key, fig)
        assert fig["summary3"] <= tolerance(case, "summary3"), (key, fig)
        sure_first = ref.gap2 > 2 * tol_d
        assert np.array_equal(sm[sure_first, 1], ref.summary[sure_first, 1].astype(np.float32)), key
        sure_count = ref.near_margin > tol_d
        assert np.array_equal(sm[sure_count, 2], ref.summary[sure_count, 2].astype(np.float32)), key
        return fig

    def _ends(self, ref, caps):
        """The reference's world end points (p0, p1) [n, C, 3] of the capsules in the state of ``self.ref_state``."""
        from tests.height_scan_ref import frame_poses
        root, dof = self.ref_state
        fr = [(int(l), tuple(p0)) for l, p0, _p1, _r in caps] + [(int(l), tuple(p1)) for l, _p0, p1, _r in caps]
        p, _R = frame_poses(self.m, root, dof, fr)
        return p[:, :len(caps)], p[:, len(caps):]


_cases = {}


def shared(case, n=N, seed=12):
    if (case, n) not in _cases:
        _cases[case, n] = Case(case, n, seed)
    return _cases[case, n]


@pytest.mark.parametrize("case", pr.CASES)
def test_outputs_match_the_reference(case):
    c = shared(case)
    ref = c.reference()
    got = c.call()
    c.check("all", got, ref, quota=case != "kat_free")
    if case == "kat_free":
        _caps, _pairs, want = pr.known_capsules()
        assert len(c.caps) == abi.TG_PROX_MAX_CAPSULES                      # C = 32
        keep = ref.keep_dist[0]
        assert np.abs(got[0][:, keep] - want[keep]).max() <= tolerance(case, "dist")
    if case == "thormang":
        assert (len(c.caps), len(c.pairs)) == (15, 99)
        assert (got[0][pr.CROSSED_ENV] < 0).sum() >= 3 and got[2][pr.CROSSED_ENV, 2] >= 3
        assert got[2][pr.CROSSED_ENV, 3] > 0.1


@pytest.mark.parametrize("case", ["thormang", "gogoro", "jit_walker"])
def test_the_far_twin_has_the_same_bits(case):
    c = shared(case)
    d, w, sm = c.call()
    assert np.array_equal(_bits(d[1]), _bits(d[0])) and np.array_equal(_bits(sm[1]), _bits(sm[0]))
    shift = c.root[1, :3].astype(np.float64) - c.root[0, :3].astype(np.float64)
    assert np.linalg.norm(shift[:2]) > 45.0
    moved = np.abs((w[1].astype(np.float64) - w[0].astype(np.float64)) - np.tile(shift, 2)).max()
    print({"case": case, "twin_witness": float(moved)})
    assert moved <= tolerance(case, "witness")


@pytest.mark.parametrize("case", ["thormang", "gogoro", "kat_free"])
def test_one_env(case):
    c = shared(case, 1, 13)
    c.check("one env", c.call(), c.reference(), quota=case != "kat_free")


@pytest.mark.parametrize("P", [1, 63, 64, 65, 256])
def test_pair_counts_around_the_wave_size(P):
    """P pairs of the walk's capsules, every pair of links three joints apart and its swap, cycled: one lane, one
    short of a wave, a wave, one more, and the limit of four passes."""
    from thormang_isaacgym_amd.sim import link_tree
    c = shared("thormang")
    pairs = pr.cycled_pairs(c.caps, link_tree(c.m)[0], P)
    assert len(pairs) == P == min(P, abi.TG_PROX_MAX_PAIRS)
    got = c.call(pairs=pairs)
    c.check(f"P={P}", got, c.reference(pairs=pairs), pairs=pairs)
    if P == 256:                                                            # pair 99 is pair 0 swapped
        assert pairs[99] == pairs[0][::-1]
        assert np.abs(got[0][:, 99] - got[0][:, 0]).max() <= tolerance("thormang", "dist")
        assert np.abs(got[1][:, 99, :3] - got[1][:, 0, 3:]).max() <= tolerance("thormang", "witness")


def test_two_capsules_and_one_pair():
    c = shared("thormang")
    caps = [c.caps[6], c.caps[12]]                                          # the thighs
    got = c.call(caps=caps, pairs=[(0, 1)])
    c.check("C=2", got, c.reference(caps=caps, pairs=[(0, 1)]), caps=caps, pairs=[(0, 1)])
    assert np.array_equal(got[2][:, 1], np.zeros(N, np.float32))


@pytest.mark.parametrize("case", ["thormang", "jit_walker"])
def test_every_combination_of_null_outputs(case):
    c = shared(case)
    full = c.call()
    names = ("dist", "witness", "summary")
    for mask in range(1, 8):
        want = tuple(n for k, n in enumerate(names) if mask >> k & 1)
        got = c.call(want=want)
        for k, n in enumerate(names):
            if n in want:
                assert np.array_equal(_bits(got[k]), _bits(full[k])), (want, n)
            else:
                assert np.isnan(got[k]).all(), (want, n)


@pytest.mark.parametrize("case", ["thormang", "gogoro"])
def test_two_identical_calls_have_the_same_bits(case):
    c = shared(case)
    a, b = c.call(), c.call()
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def test_runtime_loaded_model():
    """jit_walker is compiled at run time (tg_model_jit): the call works, no TG_ERR_MODEL."""
    from thormang_isaacgym_amd.sim import compiled_model_hashes
    c = shared("jit_walker")
    assert c.s.jit and abi.ModelDesc(c.m).hash not in compiled_model_hashes()
    c.check("jit", c.call(), c.reference())


@pytest.mark.parametrize("case", ["thormang", "gogoro"])
def test_a_call_after_a_step_reads_the_new_state(case):
    c = Case(case, seed=14)
    s = c.s
    first = c.call()
    c.check("first", first, c.reference())
    s.root_state[:, 2] += 0.5                   # clear of the ground: the step is a short free flight
    s.dof_state.view(c.n, s.D, 2)[:, :, 1] = 0.8
    s.simulate()
    torch.cuda.synchronize()
    root, dof = s.root_state.cpu().numpy().copy(), s.dof_state.cpu().numpy().copy()
    assert not np.array_equal(dof, c.dof)
    second = c.call()
    c.ref_state = (root, dof)
    c.check("after a step", second, c.reference(root=root, dof=dof))
    assert not np.array_equal(first[0], second[0])


def test_wrapper_returns_the_named_tuple_and_checks_its_arguments():
    c = shared("thormang")
    s = c.s
    caps = pr.as_structs(c.caps)
    pairs = s.capsule_pairs(caps)
    assert pairs == c.pairs
    want = c.call()
    got = s.proximity(caps, pairs, margin=MARGIN, dist=True, witness=True, summary=True)
    torch.cuda.synchronize()
    assert type(got).__name__ == "Proximity" and got._fields == ("dist", "witness", "summary")
    for x, y in zip(got, want):
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(y))
    only = s.proximity(caps, pairs)
    assert only.witness is None and only.summary is None and tuple(only.dist.shape) == (N, len(pairs))
    given = _nan(N, 4)
    assert s.proximity(caps, pairs, margin=MARGIN, dist=False, summary=True, out_summary=given).summary is given
    torch.cuda.synchronize()
    assert np.array_equal(_bits(given.cpu().numpy()), _bits(want[2]))
    thigh = s.limb_capsule("l_leg_hip_p_link", "l_leg_kn_p_link", 0.06)
    assert np.allclose(list(thigh.p1), [0.0, 0.06, -0.3], atol=1e-7) and thigh.link == c.caps[6][0]
    assert s.capsule("pelvis_link", (0, 0, 0.1)).link == 0 and list(s.capsule(0, (0, 0, 0.5)).p1) == [0.0, 0.0, 0.5]
    with pytest.raises(ValueError):
        s.limb_capsule("l_leg_hip_p_link", "l_leg_an_p_link", 0.05)
    with pytest.raises(ValueError):
        s.proximity(caps, pairs, out=torch.zeros(N, len(pairs) + 1, device="cuda:0"))
    with pytest.raises(ValueError):
        s.proximity(caps, [(0, 0)])
    with pytest.raises(ValueError):
        s.proximity(caps, [(0, len(caps))])
    with pytest.raises(ValueError):
        s.proximity(caps, pairs, dist=False)
    with pytest.raises(ValueError):
        s.proximity(caps, pairs, margin=float("nan"))
    with pytest.raises(ValueError):
        s.proximity(caps * 3, pairs)


# ------------------------------------------------------------------ the walk task

def _walk(n, on, noise=None, contact_forces=False):
    """``on``: None builds the task without the key, False and True with ``enableSelfProximity`` set to it."""
    from tests.gpu_harness import NumpyDraws, make_gpu_walk, walk_cfg
    cfg = walk_cfg(n)
    if on is not None:
        cfg["env"]["enableSelfProximity"] = on
    if noise is not None:
        cfg["env"]["jointNoise"] = noise
    if contact_forces:
        cfg["env"]["enableContactForces"] = True
    return make_gpu_walk(cfg, NumpyDraws(5))


def test_walk_task_exposes_the_summary_and_is_otherwise_unchanged():
    """ThormangWalk, 16 envs, 12 steps of fixed actions: a task built without the key, one with env.enableSelfProximity
    false and one with it true.  Obs, reward, reset and the sim state of all three are bit-identical and the first two
    carry no extras key; extras["self_proximity"] is sim.proximity(...).summary of the state the step returned with,
    and matches the reference on the state read back."""
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from thormang_isaacgym_amd.tasks.thormang_walk import WALK_SELF_MARGIN
    n = 16
    off, flag_off, on = _walk(n, None), _walk(n, False), _walk(n, True)
    D = on.model.num_dof
    for env in (off, flag_off):
        assert env.self_proximity is None and "self_proximity" not in env.extras
    assert "enableSelfProximity" not in off.cfg["env"] and flag_off.cfg["env"]["enableSelfProximity"] is False
    caps, pairs = on.self_capsules, on.self_pairs
    assert on.self_margin == WALK_SELF_MARGIN and (len(caps), len(pairs)) == (15, 99)
    act = torch.from_numpy(np.random.default_rng(9).uniform(-0.5, 0.5, (n, D)).astype(np.float32)).cuda()
    worst = {"summary0": 0.0, "summary3": 0.0}
    for k in range(12):
        o0, r0, z0, x0 = off.step(act.clone())
        o1, r1, z1, x1 = on.step(act.clone())
        o2, r2, z2, x2 = flag_off.step(act.clone())
        assert torch.equal(o0["obs"], o2["obs"]) and torch.equal(r0, r2) and torch.equal(z0, z2)
        assert torch.equal(x0["time_outs"], x2["time_outs"]) and "self_proximity" not in x2 and set(x0) == set(x2)
        assert torch.equal(o0["obs"], o1["obs"]) and torch.equal(r0, r1) and torch.equal(z0, z1)
        assert torch.equal(x0["time_outs"], x1["time_outs"]) and "self_proximity" not in x0
        sp = x1["self_proximity"]
        assert tuple(sp.shape) == (n, 4) and bool(torch.isfinite(sp).all())
        kept = sp.clone()
        again = on.sim.proximity(caps, pairs, margin=WALK_SELF_MARGIN, dist=False, summary=True).summary
        assert torch.equal(again, kept)
        assert torch.equal(on.proximity(caps, pairs, margin=WALK_SELF_MARGIN, dist=False, summary=True).summary, kept)
        if k % 4 == 3:
            torch.cuda.synchronize()
            ref = pr.proximity_ref(on.model, on.sim.root_state.cpu().numpy(), on.sim.dof_state.cpu().numpy(),
                                   pr.capsule_tuples(caps), pairs, WALK_SELF_MARGIN)
            got = kept.cpu().numpy()
            ok = ref.keep_dist.all(axis=1)
            worst["summary0"] = max(worst["summary0"], float(np.abs(got[:, 0] - ref.summary[:, 0])[ok].max()))
            worst["summary3"] = max(worst["summary3"],
                                    float(np.abs(got[:, 3] - ref.summary[:, 3])[ok].max()) / len(pairs))
    print({"case": "walk_task", **worst})
    assert worst["summary0"] <= tolerance("walk_task", "summary0")
    assert worst["summary3"] <= tolerance("walk_task", "summary3")
    for env in (flag_off, on):
        assert torch.equal(off.sim.root_state, env.sim.root_state) and torch.equal(off.sim.dof_state, env.sim.dof_state)


def test_walk_tasks_default_stance_reads_a_count_of_zero():
    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    from thormang_isaacgym_amd.tasks.thormang_walk import WALK_SELF_MARGIN
    env = _walk(4, True, noise=0.0, contact_forces=True)    # (beside another optional extra)
    assert "feet_contact_force" in env.extras
    got = env.sim.proximity(env.self_capsules, env.self_pairs, margin=WALK_SELF_MARGIN, summary=True)
    torch.cuda.synchronize()
    sm = got.summary.cpu().numpy()
    assert (sm[:, 2] == 0).all() and (sm[:, 3] == 0).all() and (sm[:, 0] >= WALK_SELF_MARGIN).all()
    assert (got.dist.cpu().numpy() >= WALK_SELF_MARGIN).all()
