"""The float64 reference of the IMU (tests/imu_ref.py) pinned without a GPU by
answers known without it:

* a free body spinning about z at rate w with the sensor at (r, 0, 0) reads
  lin_acc_b -> (-w^2 r, 0, |g|) as dt -> 0: the point's velocity is w r
  (-sin th, cos th, 0), and its difference over dt, seen in the body axes at the
  later time, is w r (-sin(w dt), 1 - cos(w dt), 0) / dt = (-w^2 r, w^3 r dt / 2,
  0) + O(dt^2): the error is first order in dt;
* gravity_b of a body pitched by th about y is (sin th, 0, -cos th);
* a free body dropped with spin reads |lin_acc_b| = 0 (free fall) and a box at
  rest on the plane (0, 0, |g|), both through the CPU oracle's physics_step;
* the history and reset semantics of the header;
* the conditioning of the accelerations of tests/test_gpu_imu.py's own inputs.
"""
import numpy as np
import pytest

from tests import physics_models as pm
from tests.imu_ref import CASES, DT, FAR, HISTORY, WIDTH, align_quat, imu_ref, scenario, sensor_kinematics
from tests.oracle_lib import physics_step

G = 9.81


def _free_state(angle_z=0.0, wz=0.0, pitch=0.0):
    root = np.zeros((1, 13), np.float32)
    if pitch:
        root[0, 3:7] = [0.0, np.sin(pitch / 2), 0.0, np.cos(pitch / 2)]
    else:
        root[0, 3:7] = [0.0, 0.0, np.sin(angle_z / 2), np.cos(angle_z / 2)]
    root[0, 12] = wz
    return root, np.zeros((0, 2), np.float32)


def _spin_error(dt, w=3.0, r=0.4, th0=0.3):
    m = pm.free_body()
    sensors = [(0, (r, 0.0, 0.0))]
    first = imu_ref(m, *_free_state(th0, w), sensors, dt=dt)
    second = imu_ref(m, *_free_state(th0 + w * dt, w), sensors, history=first.history, dt=dt)
    assert second.out[0, 0, 19] == 1.0
    return second.out[0, 0, 13:16] - np.array([-w * w * r, 0.0, G]), second


def test_spinning_body_reads_the_centripetal_acceleration_with_first_order_convergence():
    w, r = 3.0, 0.4
    errs = {}
    for dt in (4e-3, 2e-3, 1e-3):
        err, got = _spin_error(dt, w, r)
        errs[dt] = err
        # the leading error term is w^3 r dt / 2 along the body's y; the root quaternion is an fp32 input, so each
        # velocity carries 1e-7 of rounding, divided by dt
        assert err[1] == pytest.approx(w ** 3 * r * dt / 2, rel=2e-2, abs=1e-3)
        assert abs(err[2]) < 1e-12
        # the gyro reads the spin and the velocity is tangential
        assert np.allclose(got.out[0, 0, 10:13], [0.0, 0.0, w], atol=1e-12)
        assert np.allclose(got.out[0, 0, 7:10], [0.0, w * r, 0.0], atol=1e-6)
        assert np.allclose(got.out[0, 0, 16:19], 0.0, atol=1e-12)
    n4, n2, n1 = (np.linalg.norm(errs[dt]) for dt in (4e-3, 2e-3, 1e-3))
    assert 1.8 < n4 / n2 < 2.2 and 1.8 < n2 / n1 < 2.2
    assert n1 < 0.01 * w * w * r


def test_gravity_of_a_pitched_body():
    th = 0.35
    got = imu_ref(pm.free_body(), *_free_state(pitch=th), [(0, (0.0, 0.0, 0.0))])
    assert np.allclose(got.out[0, 0, 4:7], [np.sin(th), 0.0, -np.cos(th)], atol=1e-7)
    # at rest without a history the accelerometer reads -R^T g: |g| along the world's up, seen from the body
    assert np.allclose(got.out[0, 0, 13:16], [-G * np.sin(th), 0.0, G * np.cos(th)], atol=1e-6)
    assert np.allclose(align_quat(got.out[0, 0, 0:4], np.array([0, np.sin(th / 2), 0, np.cos(th / 2)])),
                       [0, np.sin(th / 2), 0, np.cos(th / 2)], atol=1e-7)
    # a tilted gravity is normalised, zero gravity gives zero
    tilted = imu_ref(pm.free_body(), *_free_state(), [(0, (0.0, 0.0, 0.0))], gravity=(3.0, 0.0, -4.0))
    assert np.allclose(tilted.out[0, 0, 4:7], [0.6, 0.0, -0.8], atol=1e-15)
    assert np.allclose(tilted.out[0, 0, 13:16], [-3.0, 0.0, 4.0], atol=1e-15)
    zero = imu_ref(pm.free_body(), *_free_state(), [(0, (0.0, 0.0, 0.0))], gravity=(0.0, 0.0, 0.0))
    assert np.array_equal(zero.out[0, 0, 4:7], [0.0, 0.0, 0.0])


FREE_FALL_START = dict(pos=[0.3, -0.2, 5.0], spin=[1.0, -2.0, 3.0])


def free_fall_readings(steps=3):
    """(|lin_acc_b|, valid) of kat_free dropped with spin, dt 0.01, 2 substeps, on each of ``steps`` steps of the
    CPU oracle."""
    m = pm.free_body()
    desc, sp, root, dof, props, pt, vt = pm.sim(m, n=1, dt=0.01, substeps=2)
    root[0, :3] = FREE_FALL_START["pos"]
    root[0, 10:13] = FREE_FALL_START["spin"]
    sensors = [(0, (0.0, 0.0, 0.0))]                      # the centre of mass: a point off it feels the spin
    # the configured gravity; the engine holds it as fp32, 4e-7 m/s^2 off, and stores the velocity as fp32, whose
    # rounding over dt is of the same size: both stay under the bound asserted
    g = (0.0, 0.0, -G)
    hist = imu_ref(m, root, dof, sensors, gravity=g, dt=0.01).history
    out = []
    for _ in range(steps):
        physics_step(desc, sp, root, dof, props, pt, vt)
        r = imu_ref(m, root, dof, sensors, gravity=g, history=hist, dt=0.01)
        hist = r.history
        out.append((float(np.linalg.norm(r.out[0, 0, 13:16])), float(r.out[0, 0, 19])))
    return out


def test_free_fall_reads_zero():
    for norm, valid in free_fall_readings():
        print("free fall |lin_acc_b| =", norm)
        assert valid == 1.0 and norm < 1e-6


def box_at_rest_states(steps=120):
    """The root states of box_body released at z = 0.06 (1 cm above rest) over ``steps`` steps of 1/60 with 2
    substeps, after each step: the oracle's run that the rest reading is taken from."""
    m = pm.box_body()
    desc, sp, root, dof, props, pt, vt = pm.sim(m, n=1, dt=1 / 60, substeps=2)
    root[0, 2] = 0.06
    states = []
    for _ in range(steps):
        physics_step(desc, sp, root, dof, props, pt, vt)
        states.append(root.copy())
    return states


def test_box_at_rest_reads_plus_g_along_up():
    states = box_at_rest_states()
    m = pm.box_body()
    dof = np.zeros((0, 2), np.float32)
    sensors = [(0, (0.0, 0.0, 0.0))]
    hist = imu_ref(m, states[-2], dof, sensors, dt=1 / 60).history
    r = imu_ref(m, states[-1], dof, sensors, history=hist, dt=1 / 60)
    acc = r.out[0, 0, 13:16]
    print("box at rest lin_acc_b =", acc)
    assert r.out[0, 0, 19] == 1.0 and abs(float(states[-1][0, 2]) - 0.05) < 1e-6
    assert abs(acc[0]) < 1e-7 and abs(acc[1]) < 1e-7 and abs(acc[2] - G) < 1e-7
    assert np.allclose(r.out[0, 0, 4:7], [0.0, 0.0, -1.0], atol=1e-6)


def test_history_and_reset_semantics():
    m, sensors, (rootA, dofA), (rootB, dofB) = scenario("jit_walker")
    n, S = rootA.shape[0], len(sensors)
    first = imu_ref(m, rootA, dofA, sensors, dt=DT)
    assert first.out.shape == (n, S, WIDTH) and first.history.shape == (n, S, HISTORY)
    # without a history: a = alpha = 0, valid = 0, the accelerometer reads -R^T g
    g = np.array([0.0, 0.0, -G])
    assert np.array_equal(first.out[..., 19], np.zeros((n, S))) and np.array_equal(first.out[..., 16:19],
                                                                                   np.zeros((n, S, 3)))
    assert np.allclose(first.out[..., 13:16], -np.einsum("esji,j->esi", first.R, g), atol=1e-14)
    # the history holds the true world velocities, flag 1, pad 0
    assert np.array_equal(first.history[..., 0:3], first.v) and np.array_equal(first.history[..., 3:6], first.w)
    assert np.array_equal(first.history[..., 6], np.ones((n, S))) and np.array_equal(first.history[..., 7],
                                                                                     np.zeros((n, S)))
    # a history whose flag is not 1.0 is no history (zeros, and garbage with another flag)
    for flag in (0.0, 0.5, 2.0, np.nan):
        h = np.full((n, S, HISTORY), 7.0)
        h[..., 6] = flag
        assert np.array_equal(imu_ref(m, rootA, dofA, sensors, history=h, dt=DT).out, first.out)
    # a valid one is differenced
    second = imu_ref(m, rootB, dofB, sensors, history=first.history, dt=DT)
    assert np.array_equal(second.out[..., 19], np.ones((n, S)))
    a = (second.v - first.v) / DT
    assert np.allclose(second.out[..., 13:16], np.einsum("esji,esj->esi", second.R, a - g), rtol=0, atol=1e-9)
    alpha = (second.w - first.w) / DT
    assert np.allclose(second.out[..., 16:19], np.einsum("esji,esj->esi", second.R, alpha), rtol=0, atol=1e-9)
    # reset envs read as without a history, the others as without the mask; the history of all is updated
    reset = np.array([0, 1, 0, 5, 0])
    masked = imu_ref(m, rootB, dofB, sensors, history=first.history, dt=DT, reset=reset)
    fresh = imu_ref(m, rootB, dofB, sensors, dt=DT)
    assert np.array_equal(masked.out[[1, 3]], fresh.out[[1, 3]])
    assert np.array_equal(masked.out[[0, 2, 4]], second.out[[0, 2, 4]])
    assert np.array_equal(masked.history, second.history) and np.array_equal(masked.history[..., 6], np.ones((n, S)))
    # bias and noise enter the gyro and the accelerometer only, and never the history
    rs = np.random.default_rng(5)
    bias, nrm = rs.normal(0, 1, (n, S, 6)), rs.normal(0, 1, (n, S, 6))
    noisy = imu_ref(m, rootB, dofB, sensors, history=first.history, dt=DT, bias=bias, gyro_noise=0.1,
                    accel_noise=0.5, normals=nrm)
    want = second.out.copy()
    want[..., 10:13] += bias[..., 0:3] + 0.1 * nrm[..., 0:3]
    want[..., 13:16] += bias[..., 3:6] + 0.5 * nrm[..., 3:6]
    assert np.allclose(noisy.out, want, rtol=0, atol=1e-12) and np.array_equal(noisy.history, second.history)


def test_env_placement_does_not_enter():
    m, sensors, (rootA, dofA), _B = scenario("thormang")
    assert tuple(rootA[1, :3]) == FAR
    moved = rootA.copy()
    moved[:, :3] += np.array([1234.5, -987.25, 3.0], np.float32)
    a, b = imu_ref(m, rootA, dofA, sensors, dt=DT), imu_ref(m, moved, dofA, sensors, dt=DT)
    assert np.array_equal(a.out, b.out) and np.array_equal(a.history, b.history)


@pytest.mark.parametrize("case", CASES)
def test_conditioning_of_the_gpu_scenarios(case):
    """The accelerations the GPU parity test compares are differences of velocities of a few m/s over dt 0.01,
    O(100 m/s^2); rounding every velocity to fp32 moves them by far less than the parity tolerance, so that
    tolerance is not set by the conditioning."""
    m, sensors, (rootA, dofA), (rootB, dofB) = scenario(case)
    first = imu_ref(m, rootA, dofA, sensors, dt=DT)
    second = imu_ref(m, rootB, dofB, sensors, history=first.history, dt=DT)
    big = float(np.abs(second.out[..., 13:16]).max())
    assert 10.0 < big < 3000.0, big
    # the same with every velocity rounded to fp32, in the history and in the current state
    _q, R, v, w = sensor_kinematics(m, rootB, dofB, sensors)
    v32, w32 = v.astype(np.float32).astype(np.float64), w.astype(np.float32).astype(np.float64)
    h32 = first.history.astype(np.float32).astype(np.float64)
    g = np.array([0.0, 0.0, -G])
    acc32 = np.einsum("esji,esj->esi", R, (v32 - h32[..., 0:3]) / DT - g)
    alpha32 = np.einsum("esji,esj->esi", R, (w32 - h32[..., 3:6]) / DT)
    moved = max(float(np.abs(acc32 - second.out[..., 13:16]).max()) / big,
                float(np.abs(alpha32 - second.out[..., 16:19]).max()) / float(np.abs(second.out[..., 16:19]).max()))
    print({"case": case, "max |lin_acc_b|": big, "moved by fp32 velocities": moved})
    assert moved < 1e-6
