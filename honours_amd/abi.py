"""The C ABI of libpress_hip.so as Python sees it: the method ids of include/press_hip.h and PROTOS, one prototype for
every function the header declares.  load_library() applies the table; nothing else assigns a restype or argtypes.
tests/test_abi_symbols.py parses the header and compares it with the table, parameter by parameter.

Pointer parameters are c_void_p (c_char_p for `const char *`), never POINTER(T): callers pass addresses as integers,
None, byref(...) and ctypes arrays, and only c_void_p takes all of them.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PRESS_HIP_LIB", os.path.join(_HERE, "libpress_hip.so"))  # override: diagnostic builds

# include/press_hip.h enum press_hip_method
METHODS = {
    "svb12": 0, "svb12_zd": 1, "svb_zd": 2, "zstd_svb_zd": 3, "zstd_svb12_zd": 4,
    "vbe21_zd": 5, "vbbe21_zd": 6, "vbsbe21_zd": 7, "vbsse21_zd": 8,
    "shuffman_vbe21_zd": 9, "shuffman_vbbe21_zd": 10, "shuffman_vbsbe21_zd": 11,
    "shuffman_vbsse21_zd": 12, "hasgam_vbsse21_zdq": 13, "zstd_hasgam_vbsse21_zdq": 14,
    "slow5_svb_zd": 15, "rc_vbe21_zd": 16, "rcc_vbe21_zd": 17, "rccm_vbbe21_zd": 18,
}
# include/press_hip.h enum press_hip_stall_method: a family of its own (the generic batch calls do not take these ids) ...
STALL_METHODS = {"rccm_svbbe21_zd": 0, "dstall_fz_1500": 1, "dstall_fz": 2}
# ... and (2x): the ids they do take for the three, PRESS_HIP_SMETHOD_BASE + the stall method
SMETHOD_BASE = 96
SMETHODS = {name: SMETHOD_BASE + sm for name, sm in STALL_METHODS.items()}
# include/press_hip.h enum press_hip_rcf_coder / press_hip_rcf_layout: the range-coder family, every coder on every
# layout (ids of its own again; "rccdf" on "vbe21" is the reference's rccdf_vbe21_zd)
RCF_CODERS = {"rc": 0, "rcc": 1, "rccm": 2, "rccdf": 3}
RCF_LAYOUTS = {"vbe21": 0, "vbbe21": 1, "vbsbe21": 2, "vbsse21": 3}
# include/press_hip.h enum press_hip_xstage and (2w): the ids the generic calls take for every stage_layout_zd method of the
# three families - PRESS_HIP_XMETHOD_BASE + 4 * stage + layout, the three pairs that are public methods under their public id
XSTAGES = {"rc": 0, "rcc": 1, "rccm": 2, "rccdf": 3, "rice": 4, "huffman": 5}
XMETHOD_BASE = 64
XMETHODS = {"%s_%s_zd" % (s, l): METHODS.get("%s_%s_zd" % (s, l), XMETHOD_BASE + 4 * si + li)
            for s, si in XSTAGES.items() for l, li in RCF_LAYOUTS.items()}

# method -> (bound symbol, press symbol, depress symbol, calling convention)
#   "svb"    void press(in, n, out, &nout64);  void depress(in, nsamples, out, &nout64)
#   "svb_nz" as svb, depress without nout (svb12_depress)
#   "vb"     void press(in, n32, out, &nout64); void depress(in, nbytes, out, &nout32)
#   "int"    int press(...) ; int depress(in, nbytes, out, &nout32)
#   "shuff"  int press(se, ...); int depress(root, ...)
_SYMS = {
    "svb12": ("svb12_bound", "svb12_press", "svb12_depress", "svb_nz"),
    "svb12_zd": ("svb12_zd_bound", "svb12_zd_press", "svb12_zd_depress", "svb"),
    "svb_zd": ("svb_zd_bound_16", "svb_zd_press_16", "svb_zd_depress_16", "svb"),
    "zstd_svb_zd": ("zstd_svb_zd_bound_16", "zstd_svb_zd_press_16", "zstd_svb_zd_depress_16", "int"),
    "zstd_svb12_zd": ("zstd_svb12_zd_bound", "zstd_svb12_zd_press", "zstd_svb12_zd_depress", "int"),
    "vbe21_zd": ("vbe21_zd_bound_16", "vbe21_zd_press_16", "vbe21_zd_depress_16", "vb"),
    "vbbe21_zd": ("vbbe21_zd_bound_16", "vbbe21_zd_press_16", "vbbe21_zd_depress_16", "vb"),
    "vbsbe21_zd": ("vbsbe21_zd_bound_16", "vbsbe21_zd_press_16", "vbsbe21_zd_depress_16", "vb"),
    "vbsse21_zd": ("vbsse21_zd_bound_16", "vbsse21_zd_press_16", "vbsse21_zd_depress_16", "vb"),
    "shuffman_vbe21_zd": ("shuffman_vbe21_zd_bound_16", "shuffman_vbe21_zd_press_16",
                          "shuffman_vbe21_zd_depress_16", "shuff"),
    "shuffman_vbbe21_zd": ("shuffman_vbbe21_zd_bound_16", "shuffman_vbbe21_zd_press_16",
                           "shuffman_vbbe21_zd_depress_16", "shuff"),
    "shuffman_vbsbe21_zd": ("shuffman_vbsbe21_zd_bound_16", "shuffman_vbsbe21_zd_press_16",
                            "shuffman_vbsbe21_zd_depress_16", "shuff"),
    "shuffman_vbsse21_zd": ("shuffman_vbsse21_zd_bound_16", "shuffman_vbsse21_zd_press_16",
                            "shuffman_vbsse21_zd_depress_16", "shuff"),
    "hasgam_vbsse21_zdq": ("hasgam_vbsse21_zdq_bound_16", "hasgam_vbsse21_zdq_press_16",
                           "hasgam_vbsse21_zdq_depress_16", "int"),
    "zstd_hasgam_vbsse21_zdq": ("zstd_hasgam_vbsse21_zdq_bound_16", "zstd_hasgam_vbsse21_zdq_press_16",
                                "zstd_hasgam_vbsse21_zdq_depress_16", "int"),
    # BLOW5's signal codec (slow5lib svb-zd)
    "slow5_svb_zd": ("slow5_svb_zd_bound", "slow5_svb_zd_press", "slow5_svb_zd_depress", "int"),
    # vbe21 + order-0 range coder (one read per lane on the device)
    "rc_vbe21_zd": ("rc_vbe21_zd_bound_16", "rc_vbe21_zd_press_16", "rc_vbe21_zd_depress_16", "vb"),
    # ... order 1 (one read per workgroup)
    "rcc_vbe21_zd": ("rcc_vbe21_zd_bound_16", "rcc_vbe21_zd_press_16", "rcc_vbe21_zd_depress_16", "vb"),
    "rccm_vbbe21_zd": ("rccm_vbbe21_zd_bound_16", "rccm_vbbe21_zd_press_16", "rccm_vbbe21_zd_depress_16", "vb"),
}

P, S, B = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_bool
I, H, U, Q, Z = ctypes.c_int, ctypes.c_int16, ctypes.c_uint32, ctypes.c_uint64, ctypes.c_size_t
SIG = [P, P, P, U, Q]   # sig, off, n, nreads, total_samples
IN = [P, P, P, U]       # in, in_off, in_len, nreads
RECODE = [I, I, P, P, P, P, P, U, Q]  # src_method, dst_method, in, in_off, in_len, n, off, nreads, total_samples

# name -> (restype, [argtypes]), in the header's order
PROTOS = {
    "read_code_table": (B, [P, P, P]),
    "build_symbol_encoder": (None, [P, P]),
    "free_encoder": (None, [P]),
    "free_huffman_tree": (None, [P]),
    "press_hip_slow5_ptr_compress_svb_zd": (P, [P, Z, P]),
    "press_hip_slow5_ptr_depress_svb_zd": (P, [P, Z, P]),
    "press_hip_last_error": (S, []),
    "press_hip_set_device": (I, [I]),
    "press_hip_set_stream": (I, [P]),
    "press_hip_reset_stream": (I, []),
    "press_hip_get_stream": (P, []),
    "press_hip_synchronize": (I, []),
    "press_hip_load_table_file": (I, [S]),
    "press_hip_set_table": (I, [P, P]),
    "press_hip_symbol_counts": (I, SIG + [P, I]),
    "press_hip_table_from_counts": (I, [P, U, P, P]),
    "press_hip_write_table_file": (I, [S, P, P, U]),
    "press_hip_bound": (Q, [I, U]),
    "press_hip_press_batch": (I, [I] + SIG + [P, P, P, I]),
    "press_hip_press_sizes": (I, [I] + SIG + [P, I]),
    "press_hip_press_packed": (I, [I] + SIG + [P, Q, U, P, P, I]),
    "press_hip_packed_exact": (I, [I]),
    "press_hip_depress_batch": (I, [I] + IN + [P, P, P, Q, P, I]),
    "press_hip_pa_cal": (I, [P, U, P]),
    "press_hip_depress_pa_batch": (I, [I] + IN + [P, P, P, Q, P, P, I]),
    "press_hip_depress_pa_fused": (I, [I]),
    "press_hip_signal_stats": (I, SIG + [P, I]),
    "press_hip_norm_cal": (I, [P, U, P]),
    "press_hip_depress_norm_batch": (I, [I] + IN + [P, P, P, Q, P, P, I]),
    "press_hip_signal_stats_timed": (I, SIG + [P, P]),
    "press_hip_signal_quantiles": (I, SIG + [P, P, U, P, I]),
    "press_hip_scale_cal": (I, [P, U, P, P]),
    "press_hip_chunk_plan": (I, [P, U, U, U, P, P, P]),
    "press_hip_depress_chunks_batch": (I, [I] + IN + [P, Q, I, U, U, P, P, P, Q, P, P, P, I]),
    "press_hip_depress_chunks_workspace_bytes": (Q, [I, Q, U, U, U]),
    "press_hip_signal_quantiles_ranged": (I, SIG + [P, P, P, U, P, I]),
    "press_hip_signal_stats_ranged": (I, SIG + [P, P, I]),
    "press_hip_depress_chunks_trimmed_batch": (I, [I] + IN + [P, Q, I, U, U, P, P, P, P, P, Q, P, P, P, P, P, P, P, I]),
    "press_hip_depress_chunks_trimmed_workspace_bytes": (Q, [I, Q, U, U, U, I]),
    "press_hip_recode_batch": (I, RECODE + [P, P, P, P, P, I]),
    "press_hip_recode_workspace_bytes": (Q, [I, I, Q, U, I]),
    "press_hip_recode_fused": (I, [I, I]),
    "press_hip_recode_sizes": (I, RECODE + [P, P, P, I]),
    "press_hip_recode_packed": (I, RECODE + [P, Q, U, P, P, P, P, I]),
    "press_hip_recode_packed_workspace_bytes": (Q, [I, I, Q, U, I]),
    "press_hip_crc32_combine": (U, [U, U, Q]),
    "press_hip_signal_crc32": (I, SIG + [P, I]),
    "press_hip_depress_crc_batch": (I, [I] + IN + [P, P, Q, P, P, I]),
    "press_hip_verify_batch": (I, [I] + IN + [P, P, P, Q, P, P, P, I]),
    "press_hip_event_params_preset": (I, [I, P]),
    "press_hip_signal_events": (I, SIG + [P, P, P, Q, P, P, I]),
    "press_hip_events_serial_reads": (U, []),
    "press_hip_jnn_params_preset": (I, [I, P]),
    "press_hip_jnn2_params_preset": (I, [I, P]),
    "press_hip_signal_segments": (I, SIG + [P, P, P, Q, P, P, P, I]),
    "press_hip_signal_adaptor": (I, SIG + [P, P, P, I]),
    "press_hip_signal_range_stats": (I, SIG + [P, P, P, I]),
    "press_hip_prefix_params_preset": (I, [I, P]),
    "press_hip_signal_prefix": (I, SIG + [P, P, P, P, P, I]),
    "press_hip_signal_prefix_workspace_bytes": (Q, [U]),
    "press_hip_signal_tally": (I, SIG + [P, P, P, P, I]),
    "press_hip_degrade_value": (H, [H, U]),
    "press_hip_degrade_batch": (I, SIG + [U, P, I]),
    "press_hip_zstd_host_frames": (U, []),
    "press_hip_host_alloc": (P, [Q]),
    "press_hip_host_free": (None, [P]),
    "press_hip_kernel_timing": (I, [I]),
    "press_hip_kernel_times": (I, [I, P, I]),
    "press_hip_shutdown": (None, []),
    "press_hip_scratch_buffers": (U, [P]),
    "press_hip_scratch_fill": (I, [I]),
    "press_hip_stall_bound": (Q, [I, U]),
    "press_hip_stall_press_batch": (I, [I] + SIG + [P, P, P, P, I]),
    "press_hip_stall_depress_batch": (I, IN + [P, P, P, Q, P, I]),
    "press_hip_rcf_bound": (Q, [I, I, U]),
    "press_hip_rcf_press_batch": (I, [I, I] + SIG + [P, P, P, P, I]),
    "press_hip_rcf_depress_batch": (I, [I, I] + IN + [P, P, P, Q, P, I]),
    "press_hip_rice_bound": (Q, [I, U]),
    "press_hip_rice_press_batch": (I, [I] + SIG + [P, P, P, P, I]),
    "press_hip_rice_press_sizes": (I, [I] + SIG + [P, P, I]),
    "press_hip_rice_depress_batch": (I, [I] + IN + [P, P, P, Q, P, I]),
    "press_hip_rice_repairs": (I, [P]),
    "press_hip_huffman_bound": (Q, [I, U]),
    "press_hip_huffman_press_batch": (I, [I] + SIG + [P, P, P, P, I]),
    "press_hip_huffman_press_sizes": (I, [I] + SIG + [P, P, I]),
    "press_hip_huffman_depress_batch": (I, [I] + IN + [P, P, P, Q, P, I]),
    "press_hip_huffman_repairs": (I, [P]),
    "press_hip_xmethod": (I, [I, I]),
    "press_hip_xmethod_parts": (I, [I, P, P]),
    "press_hip_smethod": (I, [I]),
    "press_hip_smethod_parts": (I, [I, P]),
    "press_hip_blow5_open": (I, [S, P]),
    "press_hip_blow5_close": (None, [P]),
    "press_hip_blow5_methods": (I, [P, P, P]),
    "press_hip_blow5_next": (I, [P, U, P, Q, P, P, P, P, P]),
    "press_hip_blow5_next_pa": (I, [P, U, P, Q, P, P, P, P, P, P]),
    "press_hip_blow5_last_error": (S, []),
    "press_hip_blow5_next_records": (I, [P, U, P, Q, P, P, P, P, P, P]),
    "press_hip_blow5_create": (I, [S, P, I, I, P]),
    "press_hip_blow5_write": (I, [P, P, Q, P, Q, P, Q]),
    "press_hip_blow5_write_batch": (I, [P, U, P, P, P, P, P, P]),
    "press_hip_blow5_index": (I, [P, I]),
    "press_hip_blow5_threads": (I, [P, I]),
    "press_hip_blow5_finish": (I, [P]),
    "press_hip_blow5_deflate_sizes": (I, [P, P, Q, P, P, P, Q, U, Q, I, P, I]),
    "press_hip_blow5_deflate_batch": (I, [P, P, Q, P, P, P, Q, U, Q, I, P, Q, P, P, I]),
    "press_hip_blow5_deflate_workspace_bytes": (Q, [Q, U]),
    "press_hip_blow5_write_image": (I, [P, P, Q, U, P, P, P]),
    "press_hip_blow5_inflate_batch": (I, [P, P, P, Q, U, P, P, P, P, I]),
    "press_hip_blow5_inflate_sizes": (I, [P, P, P, Q, U, P, P, I]),
    "press_hip_blow5_inflate_packed": (I, [P, P, P, Q, U, P, Q, U, P, P, P, I]),
    "press_hip_blow5_record_fields": (I, [P, P, P, Q, U, I, P, P, P, P, P, I]),
    "press_hip_blow5_inflate_workspace_bytes": (Q, [Q, U]),
    "press_hip_blow5_next_stored": (I, [P, U, P, Q, P, P, P]),
}
for _fam in ("", "packed_", "depress_pa_", "depress_norm_", "verify_", "stall_"):  # (method, total_samples, nreads)
    PROTOS["press_hip_%sworkspace_bytes" % _fam] = (Q, [I, Q, U])
for _fam in ("events", "segments", "tally"):                                       # (total_samples, nreads)
    PROTOS["press_hip_signal_%s_workspace_bytes" % _fam] = (Q, [Q, U])

# the per-read symbols by calling convention: kind -> (bound, press, depress)
_PER_READ = {
    "svb_nz": ((Q, [Q]), (None, [P, U, P, P]), (None, [P, Q, P])),
    "svb": ((Q, [Q]), (None, [P, Q, P, P]), (None, [P, Q, P, P])),
    "vb": ((Q, [U]), (None, [P, U, P, P]), (None, [P, Q, P, P])),
    "int": ((Q, [U]), (I, [P, U, P, P]), (I, [P, Q, P, P])),
    "shuff": ((Q, [U]), (I, [P, P, U, P, P]), (I, [P, P, Q, P, P])),
}
for _syms in _SYMS.values():
    PROTOS.update(zip(_syms[:3], _PER_READ[_syms[3]]))
# the stall methods, the sixteen coder_layout_zd pairs and the four rice_layout_zd methods are called as "vb"
for _m in list(STALL_METHODS) + ["%s_%s_zd" % (c, l) for c in list(RCF_CODERS) + ["rice"] for l in RCF_LAYOUTS]:
    PROTOS.update(zip((_m + "_bound_16", _m + "_press_16", _m + "_depress_16"), _PER_READ["vb"]))
# ... and the four huffman_layout_zd methods as "int"
for _m in ["huffman_%s_zd" % l for l in RCF_LAYOUTS]:
    PROTOS.update(zip((_m + "_bound_16", _m + "_press_16", _m + "_depress_16"), _PER_READ["int"]))

# the degraded forms: plain name -> (degraded name, the leading method ids `bits` goes behind)
DEGRADED = {"recode_batch": ("recode_degraded_batch", 2), "recode_sizes": ("recode_degraded_sizes", 2),
            "recode_packed": ("recode_degraded_packed", 2), "verify_batch": ("verify_degraded_batch", 1),
            "recode_workspace_bytes": ("recode_degraded_workspace_bytes", 2),
            "recode_packed_workspace_bytes": ("recode_degraded_packed_workspace_bytes", 2)}
for _plain, (_deg, _at) in DEGRADED.items():
    _res, _args = PROTOS["press_hip_" + _plain]
    PROTOS["press_hip_" + _deg] = (_res, _args[:_at] + [U] + _args[_at:])

# every symbol include/press_hip.h declares (checked by tests/test_abi_symbols.py)
HEADER_SYMBOLS = sorted(PROTOS)

# exported for the tests only, not in the header
_UNDECLARED = {"press_hip_debug_pass_a_launches": (Q, []), "press_hip_debug_stage_sizing_launches": (Q, []),
               "press_hip_debug_stall_inner_presses": (Q, [])}
# what HuffmanTable needs of libc, and what the tests and bench.py need of libzstd
_LIBC = {"fopen": (P, [S, S]), "fclose": (I, [P]), "malloc": (P, [Z])}
ZSTD = {"ZSTD_decompress": (Z, [P, Z, P, Z]), "ZSTD_compress": (Z, [P, Z, P, Z, I]), "ZSTD_isError": (I, [Z])}


class PressError(RuntimeError):
    pass


def declare(lib, protos=PROTOS, optional=False):
    """set restype and argtypes of `lib`'s functions from a table; optional: skip what an older build does not export"""
    for name, (restype, argtypes) in protos.items():
        if optional and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    return lib


_lib = None


def load_library(path=LIB_PATH):
    """dlopen libpress_hip.so (no GPU needed for that) - raises if it is not built."""
    global _lib
    if _lib is None:
        if not os.path.exists(path):
            raise PressError("%s is not built: run `python -m honours_amd.build` "
                             "(there is no CPU fallback)" % path)
        lib = declare(declare(ctypes.CDLL(path)), _UNDECLARED)
        lib._libc = declare(ctypes.CDLL(None), _LIBC)
        _lib = lib
    return _lib
