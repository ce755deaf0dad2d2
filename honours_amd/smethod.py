"""The stall methods in the generic calls (include/press_hip.h section 2x): rccm_svbbe21_zd, dstall_fz_1500 and dstall_fz
have a method id, 96 .. 98, that press_batch, press_sizes, press_packed, recode_batch, verify_batch ... take beside the 19
public ones and the families' extended ids.  The names are abi.SMETHODS (press.SMETHODS); the wrappers of
honours_amd.press accept them as they accept the public names.  Every function here is also an attribute of
honours_amd.press (press.smethod_id ...).
"""
import ctypes

from . import abi
from . import press as _p


def smethod_id(stall_method):
    """press_hip_smethod: the id the generic calls take for a stall method (a name of abi.STALL_METHODS or 0 .. 2),
    96 + the stall method; -1 for one out of range.  Host arithmetic, no GPU"""
    sm = abi.STALL_METHODS[stall_method] if isinstance(stall_method, str) else int(stall_method)
    return int(_p.load_library().press_hip_smethod(sm))


def smethod_parts(mid):
    """press_hip_smethod_parts: the stall method (0 .. 2) of an id 96 .. 98 or a name of abi.SMETHODS; raises PressError for
    any other id"""
    sm = ctypes.c_int(-1)
    _p._call("press_hip_smethod_parts", _p._mid(mid), ctypes.byref(sm))
    return sm.value


def smethod_names():
    """the three names of abi.SMETHODS, by id"""
    return list(abi.SMETHODS)


def smethod_inner_presses():
    """how often the inner range coder of the stall methods has been launched over a batch's pieces so far: a press, a
    sizes and a packed call take it once each"""
    return int(_p.load_library().press_hip_debug_stall_inner_presses())
