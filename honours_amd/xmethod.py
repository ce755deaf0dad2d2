"""The families' methods in the generic calls (include/press_hip.h section 2w): every stage_layout_zd method of the
range-coder, Rice and per-read Huffman families has a method id that press_batch, recode_batch, verify_batch ... take
beside the 19 public ones.  The names are abi.XMETHODS (press.XMETHODS); the wrappers of honours_amd.press accept them as
they accept the public names.  Every function here is also an attribute of honours_amd.press (press.xmethod_id ...).

Stages go by name or id (abi.XSTAGES), layouts by name or id (abi.RCF_LAYOUTS).
"""
import ctypes

from . import abi
from . import press as _p


def _sid(stage):
    return abi.XSTAGES[stage] if isinstance(stage, str) else int(stage)


def _lid(layout):
    return abi.RCF_LAYOUTS[layout] if isinstance(layout, str) else int(layout)


def xmethod_id(stage, layout):
    """press_hip_xmethod: the id the generic calls take for stage_layout_zd - 16 / 17 / 18 for the three pairs that are
    public methods, else 64 + 4 * stage + layout; -1 for a bad stage or layout.  Host arithmetic, no GPU"""
    return int(_p.load_library().press_hip_xmethod(_sid(stage), _lid(layout)))


def xmethod_parts(mid):
    """press_hip_xmethod_parts: (stage, layout) of an id of xmethod_id, of 64 .. 87 or of 16 / 17 / 18; raises PressError for
    any other id"""
    stage, layout = ctypes.c_int(-1), ctypes.c_int(-1)
    _p._call("press_hip_xmethod_parts", _p._mid(mid), ctypes.byref(stage), ctypes.byref(layout))
    return stage.value, layout.value


def xmethod_names():
    """the 24 names of abi.XMETHODS, stage by stage and layout by layout"""
    return list(abi.XMETHODS)


def xmethod_sizing_launches():
    """how often a prefix-code stage's sizing kernels (Rice: count and pick; per-read Huffman: histogram and tree) have been
    launched so far: a packed press takes its sizes once"""
    return int(_p.load_library().press_hip_debug_stage_sizing_launches())
