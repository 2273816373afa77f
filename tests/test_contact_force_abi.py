"""Net contact force tensor, the parts that need no GPU: the header declares
tg_set_net_contact_force_tensor, the library exports it, the ctypes binding
has its argument types, and Sim's contact_link_indices are the links the
models' shapes sit on."""
import ctypes as C
import os
import re

import pytest

from thormang_isaacgym_amd import abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "tg_set_net_contact_force_tensor"


def test_header_declares_the_entry_point_and_its_reference_counterpart():
    text = open(os.path.join(REPO, "include", "tgsim.h")).read()
    assert re.search(r"^int\s+%s\(tg_sim \*sim, float \*out\);" % NAME, text, re.M)
    # the table of reference counterparts at the top of the header
    head = text[:text.index("#ifndef")] if "#ifndef" in text else text
    assert NAME in head and "acquire_net_contact_force_tensor" in head and "tasks/anymal.py:113,117" in head


def test_library_exports_and_binds_the_symbol():
    from thormang_isaacgym_amd import _lib
    assert os.path.exists(_lib.LIB_PATH), "libtgsim.so not built"
    assert _lib.SIGNATURES[NAME] == [C.c_void_p, C.c_void_p]
    f = getattr(_lib.lib(), NAME)
    assert f.argtypes == [C.c_void_p, C.c_void_p] and f.restype is C.c_int
    # a null sim is rejected with a message, not dereferenced
    assert f(None, None) < 0
    assert b"null tg_sim" in _lib.lib().tg_last_error()


@pytest.mark.parametrize("name", ["thormang", "thormang_wb", "gogoro", "kat_box"])
def test_contact_link_indices_are_the_shape_links(name):
    from thormang_isaacgym_amd.sim import Sim, contact_link_indices, load_model
    m = load_model(name)
    want = sorted(set(int(x) for x in abi.ModelDesc(m).arrays["shape_link"]))
    assert contact_link_indices(m) == want and len(want) > 0
    # the generated kernel traits carry the same table (the kernel's CFLinks is built from it)
    inc = open(os.path.join(REPO, "thormang_isaacgym_amd", "csrc", "generated", f"Model_{name}.inc")).read()
    arr = re.search(r"shape_link\[\d+\] = \{([^}]*)\}", inc).group(1)
    assert sorted(set(int(x) for x in arr.split(","))) == want
    # Sim exposes it as a property (no GPU needed to evaluate it on a bare instance)
    s = Sim.__new__(Sim)
    s.model = m
    assert s.contact_link_indices == want
    s._h = None


def test_task_feet_are_the_foot_links():
    from thormang_isaacgym_amd.sim import load_model
    from thormang_isaacgym_amd.tasks.thormang_walk import walk_feet_indices
    for name in ("thormang", "thormang_wb"):
        m = load_model(name)
        assert [m.links[i].name for i in walk_feet_indices(m)] == ["l_leg_foot_link", "r_leg_foot_link"]
