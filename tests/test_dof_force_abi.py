"""DOF force tensor, the parts that need no GPU: the header declares
tg_set_dof_force_tensor and lists its reference counterpart, the library
exports it, the ctypes binding has its argument types -- and the identity the
GPU tests hold the tensor to is the restated physics' own: on a driven
pendulum the fp64 oracle's inverse dynamics equal the implicit PD law at the
end-of-substep velocity."""
import ctypes as C
import os
import re

import numpy as np

from tests import physics_models as pm
from thormang_isaacgym_amd import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tg_set_dof_force_tensor"


def test_header_declares_the_entry_point_and_its_reference_counterpart():
    text = open(os.path.join(REPO, "include", "tgsim.h")).read()
    assert re.search(r"^int\s+%s\(tg_sim \*sim, float \*out\);" % NAME, text, re.M)
    # the table of reference counterparts at the top of the header
    head = text[:text.index("#ifndef")] if "#ifndef" in text else text
    assert NAME in head and "acquire_dof_force_tensor / refresh_dof_force_tensor" in head
    assert "tasks/MA_OP3.py:91,96" in head
    # the definition says what is not part of the value
    body = text[text.index("acquire_dof_force_tensor: out"):text.index("int %s(" % NAME)]
    assert "limit spring and damper are NOT part" in " ".join(body.replace("*", " ").split())


def test_library_exports_and_binds_the_symbol():
    from thormang_isaacgym_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "libtgsim.so not built"
    assert _lib.SIGNATURES[NAME] == [C.c_void_p, C.c_void_p]
    f = getattr(_lib.lib(), NAME)
    assert f.argtypes == [C.c_void_p, C.c_void_p] and f.restype is C.c_int
    # a null sim is rejected with a message, not dereferenced
    assert f(None, None) < 0
    assert b"null tg_sim" in _lib.lib().tg_last_error()


def test_python_layers_pass_the_tensor_through():
    from thormang_isaacgym_amd.sim import Sim
    from thormang_isaacgym_amd.tasks.base.vec_task import VecTask
    for cls in (Sim, VecTask):
        assert callable(cls.acquire_dof_force_tensor) and callable(cls.refresh_dof_force_tensor)


def test_oracle_inverse_dynamics_equal_the_implicit_pd_law():
    """kat_pendulum_y, fixed base, one substep, a POS drive far from
    saturation, fp64 oracle: (I_axis + armature) (qd1 - qd0) / h + m g l
    sin(q0) = te - K (qd1 - qd0) / h to 1e-9 relative, with I_axis = Ic + m
    l^2, the gravity torque at the substep's starting angle and the oracle's
    own qd0, qd1 (qd1 = qd0 + h qdd in fp64 from its dump; the float32 state it
    returns is that value rounded).  So the torque formula of tgsim.h is what
    the restated physics applies, contacts or not."""
    from tests.oracle_lib import lib as oracle_lib, physics_step
    L = oracle_lib("f64")
    L.oracle_dump_set.argtypes = [C.c_int, C.c_int]
    L.oracle_dump_read.argtypes = [C.c_void_p, C.c_int]
    l, mass, Ic = 0.5, 1.0, 0.01
    m = pm.pendulum(l=l, mass=mass, Ic=Ic)
    assert m.name == "kat_pendulum_y"
    Ic = float(np.float32(Ic))   # (the model description and the sim parameters are float32)
    rs = np.random.default_rng(3)
    worst = 0.0
    for _ in range(8):
        desc, sp, root, dof, props, pt, vt = pm.sim(m, n=1, dt=0.01, substeps=1, fix_base_link=True)
        props[abi.TG_PROP_DRIVE_MODE] = 1
        props[abi.TG_PROP_STIFFNESS] = rs.uniform(20, 200)
        props[abi.TG_PROP_DAMPING] = rs.uniform(1, 10)
        props[abi.TG_PROP_EFFORT] = 1e30
        props[abi.TG_PROP_ARMATURE] = rs.uniform(0.0, 0.05)
        dof[0] = rs.uniform(-1.5, 1.5), rs.uniform(-3, 3)
        pt[0, 0], vt[0, 0] = rs.uniform(-1, 1), rs.uniform(-1, 1)
        q0, qd0 = float(dof[0, 0]), float(dof[0, 1])
        kp, kd, arm = (float(props[k, 0, 0]) for k in (abi.TG_PROP_STIFFNESS, abi.TG_PROP_DAMPING,
                                                       abi.TG_PROP_ARMATURE))
        h, g = float(sp.dt), -float(sp.gravity[2])
        L.oracle_dump_set(0, 0)
        try:
            physics_step(desc, sp, root, dof, props, pt, vt, threads=1, L=L)
            buf = np.zeros(4096)
            L.oracle_dump_read(buf.ctypes.data, 4096)
        finally:
            L.oracle_dump_set(-1, 0)
        assert buf[2790] == 0, "the drive is far from saturation"
        qdd = float(buf[2800])
        qd1 = qd0 + h * qdd
        assert abs(float(dof[0, 1]) - qd1) <= np.spacing(np.float32(abs(qd1))), "the returned state is qd1 rounded"
        te = kp * (float(pt[0, 0]) - q0 - h * qd0) + kd * (float(vt[0, 0]) - qd0)
        K = h * kd + h * h * kp
        lhs = (Ic + mass * l * l + arm) * (qd1 - qd0) / h + mass * g * l * np.sin(q0)
        rhs = te - K * (qd1 - qd0) / h
        rel = abs(lhs - rhs) / max(abs(lhs), abs(rhs), abs(te))
        worst = max(worst, rel)
        assert rel <= 1e-9, (lhs, rhs, rel)
    print("inverse dynamics vs implicit PD law, fp64 oracle: worst relative difference %.2e" % worst)
