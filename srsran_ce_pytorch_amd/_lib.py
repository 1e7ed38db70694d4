"""ctypes binding of libce_hip.so (C ABI: include/ce_hip.h) and the in-tree build recipe.

The product path has no CPU fallback: if the library is missing or fails to load,
``load()`` raises and every estimator entry point with it.
"""
from __future__ import annotations

import ctypes as C
import os
import shutil
import subprocess
from pathlib import Path
from typing import NamedTuple

PKG_DIR = Path(__file__).resolve().parent
CSRC = PKG_DIR / "csrc"
INCLUDE = PKG_DIR.parent / "include"
LIB_PATH = Path(os.environ.get("CE_HIP_LIB", CSRC / "libce_hip.so"))   # override: diagnostic builds (tools/)
# the same library with the tuning / A-B knobs of include/ce_hip.h compiled in (-DCE_TUNING_KNOBS: environment variables
# read at plan creation).  Diagnostic only -- tests/test_hip_tiers.py and the dev tools load it through CE_HIP_LIB; the
# shipped libce_hip.so never reads the environment.
KNOBS_LIB_PATH = CSRC / "libce_hip_knobs.so"
# the estimation kernel template (ce_estimate_kernel.h) is instantiated in slices, one translation unit each, so the
# units compile concurrently (ce_inst.inc)
SOURCES = ["ce_api.hip", "ce_denoise.hip", "ce_dmrs.hip", "ce_dmrs_lp.hip", "ce_eq.hip", "ce_demod.hip", "ce_rm.hip", "ce_tp.hip", "ce_ofdm.hip", "ce_chan.hip", "ce_fh.hip", "ce_prach.hip", "ce_srs.hip", "ce_ldpc.hip", "ce_tb.hip", "ce_enc.hip", "ce_mod.hip", "ce_inst_reg_h1_f0.hip", "ce_inst_reg_h1_f1.hip", "ce_inst_reg_h1_f1w.hip", "ce_inst_reg_h2_f0.hip",
           "ce_inst_reg_h2_f1.hip", "ce_inst_gen_h1.hip", "ce_inst_gen_h2.hip", "ce_inst_narrow.hip"]


def build_deps() -> list[Path]:
    """What build() compares the libraries' age with: every source and header of csrc/, everything under include/, this file."""
    return sorted(p for pat in ("*.hip", "*.h", "*.inc") for p in CSRC.glob(pat)) + sorted(p for p in INCLUDE.rglob("*") if p.is_file()) + [Path(__file__)]


class Header(NamedTuple):
    """One public header of include/: the ctypes mirror of every structure it defines, by its C name, and
    entry point -> (restype, argtypes) for every function it declares."""
    structs: dict
    signatures: dict


# The public headers in the order load() applies them; a stage registers here and in SOURCES, nowhere else
# (tests/test_abi_conformance.py holds every entry against its header and the compiler's record layouts).
REGISTRY: dict[str, Header] = {}
CE_ABI_VERSION = 3
CE_MAX_CDM, CE_MAX_HOPS, CE_MAX_SYMBOLS = 2, 2, 14
SMOOTHING = {"none": 0, "mean": 1, "filter": 2, "mmse": 3}   # "mmse": extension, not in the reference
INTERP = {"linear": 0, "cnn": 1}
CE_ERR_INVALID, CE_ERR_UNSUPPORTED, CE_ERR_HIP, CE_ERR_NOMEM = -1, -2, -3, -4


class HopDesc(C.Structure):
    _fields_ = [("dmrs_symbols", C.c_uint8 * CE_MAX_SYMBOLS), ("re_mask", C.c_uint16 * CE_MAX_CDM),
                ("prb_start", C.c_int32), ("n_prbs", C.c_int32), ("mask_prbs", C.POINTER(C.c_uint8)),
                ("start_symbol", C.c_int32), ("n_alloc_symbols", C.c_int32)]


class PlanDesc(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("device", C.c_int32), ("n_prb_grid", C.c_int32), ("n_sym", C.c_int32),
                ("n_layers", C.c_int32), ("n_hops", C.c_int32), ("smoothing", C.c_int32),
                ("cfo_compensate", C.c_int32), ("interp", C.c_int32), ("reserved0", C.c_int32),
                ("scs_hz", C.c_double), ("beta_dmrs", C.c_double), ("cp_ms", C.c_double * CE_MAX_SYMBOLS),
                ("cnn_smoothing_alpha", C.c_double), ("mmse_delay_spread_s", C.c_double),
                ("mmse_noise_to_signal", C.c_double), ("hop", HopDesc * CE_MAX_HOPS)]


class PlanInfo(C.Structure):
    _fields_ = [("n_sc", C.c_int32), ("n_re", C.c_int32), ("n_dmrs_total", C.c_int32), ("cfo_estimated", C.c_int32),
                ("lds_bytes", C.c_int32), ("threads", C.c_int32), ("alg_bytes_per_item", C.c_int64),
                ("pilot_bytes_per_slot", C.c_int64)]


class PlanHostView(C.Structure):
    _fields_ = [("n_re", C.c_int32), ("n_dmrs_total", C.c_int32), ("n_pils", C.c_int32), ("rc_len", C.c_int32),
                ("reg_nd", C.c_int32), ("lds_bytes", C.c_int32), ("scratch_bytes", C.c_int32), ("filt_windowed", C.c_int32),
                ("cfo_estimated", C.c_int32), ("narrow", C.c_int32),
                ("ta_nres", C.c_int32 * CE_MAX_HOPS), ("contig", C.c_int32 * CE_MAX_HOPS),
                ("last_idx", (C.c_int32 * CE_MAX_CDM) * CE_MAX_HOPS),
                ("r_ord", ((C.c_int32 * 12) * CE_MAX_CDM) * CE_MAX_HOPS),
                ("alpha", ((C.c_float * 12) * CE_MAX_CDM) * CE_MAX_HOPS),
                ("rc", C.c_double * 31), ("sst", C.c_double * CE_MAX_SYMBOLS), ("two_pi_nsamples", C.c_double * CE_MAX_HOPS),
                ("n_pilots", C.c_double), ("noise_den", C.c_double), ("mmse_w", ((C.c_float * 32) * 32) * 2),
                ("reg_kpt", C.c_int32), ("feat", C.c_int32), ("ta_lp", C.c_int32), ("ta_over_p", C.c_int32),
                ("pil_stash", C.c_int32), ("sym_overlap", C.c_int32), ("cnn_comb2", C.c_int32),
                ("kernel_unit", C.c_int32), ("kernel_key", C.c_int32)]


# PlanHostView.kernel_unit (CE_UNIT_* of include/ce_hip.h) -> the instantiation unit's source
KERNEL_UNITS = ["ce_inst_narrow.hip", "ce_inst_reg_h1_f0.hip", "ce_inst_reg_h1_f1.hip", "ce_inst_reg_h1_f1w.hip",
                "ce_inst_reg_h2_f0.hip", "ce_inst_reg_h2_f1.hip", "ce_inst_gen_h1.hip", "ce_inst_gen_h2.hip"]


_int, _vp, _i64, _i32 = C.c_int, C.c_void_p, C.c_int64, C.c_int32
_i64p, _fp, _P = C.POINTER(C.c_int64), C.POINTER(C.c_float), C.POINTER
_BATCH = [_vp, _vp, _i64p, _vp, _i64p, _i64, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
REGISTRY["ce_hip.h"] = Header(structs={"ce_hop_desc": HopDesc, "ce_plan_desc": PlanDesc, "ce_plan_info": PlanInfo, "ce_plan_host_view": PlanHostView}, signatures={
    "ce_plan_create": (_int, [_P(PlanDesc), _P(_vp)]),
    "ce_plan_destroy": (None, [_vp]),
    "ce_plan_get_info": (_int, [_vp, _P(PlanInfo)]),
    "ce_plan_derive_host": (_int, [_P(PlanDesc), _P(PlanHostView)]),
    "ce_estimate_batch": (_int, _BATCH),
    "ce_estimate_batch_stages": (_int, _BATCH[:-1] + [_vp, _vp, _vp]),
    "ce_time_batch": (_int, _BATCH + [_i32, _i32, _P(C.c_double)]),
    "ce_last_error": (C.c_char_p, []),
    "ce_abi_version": (_int, []),
})
REGISTRY["ce_denoise.h"] = Header(structs={}, signatures={   # extension
    "ce_denoiser_create": (_int, [_i32, _fp, _fp, _fp, _fp, _fp, _fp, _P(_vp)]),
    "ce_denoiser_destroy": (None, [_vp]),
    "ce_denoise_batch": (_int, [_vp, _vp, _i64, _i32, _i32, _i32, _vp]),
})
CE_DMRS_MAX_WORDS, CE_DMRS_MAX_RE = 136, 2048
CE_DMRS_LP_HOP_NEITHER, CE_DMRS_LP_HOP_GROUP, CE_DMRS_LP_HOP_SEQUENCE, CE_DMRS_LP_MAX_WORDS, CE_DMRS_LP_INFO_LEN = 0, 1, 2, 560, 8
CE_DMRS_LP_FORM_ZC, CE_DMRS_LP_FORM_30, CE_DMRS_LP_FORM_PHI = 0, 1, 2


class DmrsHopDesc(C.Structure):
    _fields_ = [("dmrs_symbols", C.c_uint8 * CE_MAX_SYMBOLS), ("re_mask", C.c_uint16 * CE_MAX_CDM),
                ("mask_prbs", C.POINTER(C.c_uint8))]


class DmrsDesc(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("device", C.c_int32), ("n_prb_grid", C.c_int32), ("grid_start_crb", C.c_int32),
                ("n_sym", C.c_int32), ("n_symb_slot", C.c_int32), ("n_layers", C.c_int32), ("n_hops", C.c_int32),
                ("hop", DmrsHopDesc * CE_MAX_HOPS)]


class DmrsInfo(C.Structure):
    _fields_ = [("n_re", C.c_int32), ("n_dmrs_total", C.c_int32), ("bytes_per_slot", C.c_int64)]


class DmrsHostView(C.Structure):
    _fields_ = [("n_re", C.c_int32), ("n_dmrs_total", C.c_int32), ("ppp", C.c_int32), ("reserved0", C.c_int32),
                ("col_hop", C.c_int32 * CE_MAX_SYMBOLS), ("col_sym", C.c_int32 * CE_MAX_SYMBOLS),
                ("word0", C.c_int32 * CE_MAX_HOPS), ("n_words", C.c_int32 * CE_MAX_HOPS),
                ("x1", (C.c_uint32 * CE_DMRS_MAX_WORDS) * CE_MAX_HOPS),
                ("t", ((C.c_uint32 * CE_DMRS_MAX_WORDS) * 31) * CE_MAX_HOPS),
                ("m", (C.c_int32 * CE_DMRS_MAX_RE) * CE_MAX_HOPS),
                ("odd_sign", (C.c_uint8 * CE_DMRS_MAX_RE) * CE_MAX_HOPS)]


REGISTRY["ce_dmrs.h"] = Header(structs={"ce_dmrs_hop_desc": DmrsHopDesc, "ce_dmrs_desc": DmrsDesc, "ce_dmrs_info": DmrsInfo, "ce_dmrs_host_view": DmrsHostView}, signatures={   # extension
    "ce_dmrs_derive_host": (_int, [_P(DmrsDesc), _P(DmrsHostView)]),
    "ce_dmrs_plan_create": (_int, [_P(DmrsDesc), _P(_vp)]),
    "ce_dmrs_plan_destroy": (None, [_vp]),
    "ce_dmrs_plan_get_info": (_int, [_vp, _P(DmrsInfo)]),
    "ce_dmrs_generate": (_int, [_vp, _vp, _vp, _vp, _i64p, _i64, _vp, _vp]),
    # low-PAPR (Zadoff-Chu) DM-RS: scalars and pointers only, the host view goes out through caller-provided arrays
    "ce_dmrs_lp_derive_host": (_int, [_i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ce_dmrs_lp_copy_twiddles": (_int, [_i32, _vp]),
    "ce_dmrs_lp_plan_create": (_int, [_i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _P(_vp)]),
    "ce_dmrs_lp_plan_destroy": (None, [_vp]),
    "ce_dmrs_lp_generate": (_int, [_vp, _vp, _i64, _vp, _i64, _i64, _vp, _vp]),
})
CE_EQ_MAX_PORTS, CE_EQ_CHUNK_SC = 8, 36


class EqHopDesc(C.Structure):
    _fields_ = [("dmrs_symbols", C.c_uint8 * CE_MAX_SYMBOLS), ("reserved_re_mask", C.c_uint16), ("prb_start", C.c_int32),
                ("n_prbs", C.c_int32), ("start_symbol", C.c_int32), ("n_alloc_symbols", C.c_int32)]


class EqDesc(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("device", C.c_int32), ("n_prb_grid", C.c_int32), ("n_sym", C.c_int32),
                ("n_layers", C.c_int32), ("n_hops", C.c_int32), ("hop", EqHopDesc * CE_MAX_HOPS)]


class EqInfo(C.Structure):
    _fields_ = [("n_data_re", C.c_int32), ("reserved0", C.c_int32), ("bytes_per_slot", C.c_int64)]


class EqHostView(C.Structure):
    _fields_ = [("sym_hop", C.c_int32 * CE_MAX_SYMBOLS), ("data_mask", C.c_int32 * CE_MAX_SYMBOLS),
                ("data_res_per_prb", C.c_int32 * CE_MAX_SYMBOLS), ("first_row", C.c_int32 * CE_MAX_SYMBOLS),
                ("n_data_re", C.c_int32)]


REGISTRY["ce_eq.h"] = Header(structs={"ce_eq_hop_desc": EqHopDesc, "ce_eq_desc": EqDesc, "ce_eq_info": EqInfo, "ce_eq_host_view": EqHostView}, signatures={   # extension
    "ce_eq_derive_host": (_int, [_P(EqDesc), _P(EqHostView)]),
    "ce_eq_plan_create": (_int, [_P(EqDesc), _P(_vp)]),
    "ce_eq_plan_destroy": (None, [_vp]),
    "ce_eq_plan_get_info": (_int, [_vp, _P(EqInfo)]),
    "ce_eq_equalize": (_int, [_vp, _vp, _i64p, _vp, _vp, _i64, _i32, _vp, _vp, _vp]),
})
CE_DEMOD_MAX_BITS, CE_DEMOD_BLOCK_WORDS, CE_DEMOD_TILE_SYMBOLS = 1 << 21, 8, 1024
CE_DEMOD_OUT_F32, CE_DEMOD_OUT_I8 = 0, 1


class DemodDesc(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("device", C.c_int32), ("qm", C.c_int32), ("out_format", C.c_int32),
                ("descramble", C.c_int32), ("n_symbols", C.c_int32), ("llr_scale", C.c_float)]


class DemodInfo(C.Structure):
    _fields_ = [("n_bits", C.c_int32), ("out_elem_bytes", C.c_int32), ("bytes_per_slot", C.c_int64)]


class DemodHostView(C.Structure):
    _fields_ = [("n_bits", C.c_int32), ("n_words", C.c_int32), ("block_words", C.c_int32), ("n_blocks", C.c_int32),
                ("tile_symbols", C.c_int32), ("n_tiles", C.c_int32), ("table_bytes", C.c_int64)]


REGISTRY["ce_demod.h"] = Header(structs={"ce_demod_desc": DemodDesc, "ce_demod_info": DemodInfo, "ce_demod_host_view": DemodHostView}, signatures={   # extension
    "ce_demod_derive_host": (_int, [_P(DemodDesc), _P(DemodHostView)]),
    "ce_demod_copy_tables": (_int, [_P(DemodDesc), _vp, _vp]),
    "ce_demod_plan_create": (_int, [_P(DemodDesc), _P(_vp)]),
    "ce_demod_plan_destroy": (None, [_vp]),
    "ce_demod_plan_get_info": (_int, [_vp, _P(DemodInfo)]),
    "ce_demod_demap": (_int, [_vp, _vp, _vp, _vp, _vp, _i64p, _i64, _vp, _vp]),
})
CE_RM_F32, CE_RM_I8, CE_RM_MAX_SLOT_ELEMS, CE_RM_TILE_UNITS = 0, 1, 1 << 24, 1024


class RmDesc(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("device", C.c_int32), ("base_graph", C.c_int32), ("tbs", C.c_int32),
                ("qm", C.c_int32), ("n_layers", C.c_int32), ("g_bits", C.c_int32), ("format", C.c_int32),
                ("n_ref", C.c_int32), ("filler_llr", C.c_float)]


class RmInfo(C.Structure):
    _fields_ = [("n_code_blocks", C.c_int32), ("n_cb", C.c_int32), ("elem_bytes", C.c_int32), ("reserved0", C.c_int32),
                ("bytes_per_slot", C.c_int64)]


class RmHostView(C.Structure):
    _fields_ = [("b", C.c_int32), ("k_cb", C.c_int32), ("c", C.c_int32), ("b_prime", C.c_int32), ("k_prime", C.c_int32),
                ("k_b", C.c_int32), ("zc", C.c_int32), ("k", C.c_int32), ("n", C.c_int32), ("n_cb", C.c_int32),
                ("f0", C.c_int32), ("f1", C.c_int32), ("p", C.c_int32), ("n_lo", C.c_int32), ("e_lo", C.c_int32),
                ("e_hi", C.c_int32), ("k0", C.c_int32 * 4), ("s", C.c_int32 * 4), ("unit_elems", C.c_int32),
                ("tiles_per_block", C.c_int32), ("n_tiles", C.c_int32)]


REGISTRY["ce_rm.h"] = Header(structs={"ce_rm_desc": RmDesc, "ce_rm_info": RmInfo, "ce_rm_host_view": RmHostView}, signatures={   # extension
    "ce_rm_derive_host": (_int, [_P(RmDesc), _P(RmHostView)]),
    "ce_rm_plan_create": (_int, [_P(RmDesc), _P(_vp)]),
    "ce_rm_plan_destroy": (None, [_vp]),
    "ce_rm_plan_get_info": (_int, [_vp, _P(RmInfo)]),
    "ce_rm_recover": (_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp]),
})
CE_TP_MAX_PRBS, CE_TP_MAX_PASSES = 275, 8


class TpDesc(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("device", C.c_int32), ("n_prbs", C.c_int32), ("n_symbols", C.c_int32)]


class TpInfo(C.Structure):
    _fields_ = [("m_sc", C.c_int32), ("n_symbols", C.c_int32), ("bytes_per_slot", C.c_int64)]


class TpHostView(C.Structure):
    _fields_ = [("m_sc", C.c_int32), ("n_passes", C.c_int32), ("radix", C.c_int32 * CE_TP_MAX_PASSES),
                ("stride_magic", C.c_uint32 * CE_TP_MAX_PASSES), ("threads_per_row", C.c_int32),
                ("rows_per_workgroup", C.c_int32), ("threads", C.c_int32), ("lds_bytes", C.c_int32),
                ("twiddle_bytes", C.c_int32), ("n_workgroups_per_slot", C.c_int32)]


REGISTRY["ce_tp.h"] = Header(structs={"ce_tp_desc": TpDesc, "ce_tp_info": TpInfo, "ce_tp_host_view": TpHostView}, signatures={   # extension
    "ce_tp_derive_host": (_int, [_P(TpDesc), _P(TpHostView)]),
    "ce_tp_copy_twiddles": (_int, [_P(TpDesc), _vp]),
    "ce_tp_plan_create": (_int, [_P(TpDesc), _P(_vp)]),
    "ce_tp_plan_destroy": (None, [_vp]),
    "ce_tp_plan_get_info": (_int, [_vp, _P(TpInfo)]),
    "ce_tp_deprecode": (_int, [_vp, _vp, _vp, _i64, _vp, _vp, _vp]),
    "ce_tp_precode": (_int, [_vp, _vp, _i64, _P(_i32), _vp, _i64, _P(_i32), _i64, _vp]),
    # OFDM demodulation: scalars and pointers only, the host view is the transforms' (m_sc holds n_fft)
    "ce_ofdm_derive_host": (_int, [_i32, _i32, _i32, _P(_i32), _i32, _P(TpHostView)]),
    "ce_ofdm_copy_twiddles": (_int, [_i32, _vp]),
    "ce_ofdm_plan_create": (_int, [_i32, _i32, _i32, _i32, _i32, _P(_i32), _i32, _fp, _P(_vp)]),
    "ce_ofdm_plan_destroy": (None, [_vp]),
    "ce_ofdm_demodulate": (_int, [_vp, _vp, _i64, _i64, _i64, _i64, _vp, _vp]),
    # OFDM modulation on the demodulator's plan (the name keeps clear of the ce_ofdm_ prefix)
    "ce_ofdmtx_modulate": (_int, [_vp, _vp, _i64, _i64, _vp, _i64, _i64, _vp]),
    # the time-domain channel emulator: no plan, scalars and pointers only
    "ce_chan_apply": (_int, [_i32, _vp, _i64, _i64, _i64, _i32, _i64, _i64, _vp, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _i64,
                             C.c_uint64, _i64, _vp, _i64, _i64, _vp]),
    "ce_chan_noise_words": (_int, [C.c_uint64, _i64, _i32, _i64, _P(C.c_uint32)]),
    # fronthaul I/Q (de)compression: no plan, scalars and pointers only
    "ce_fh_row_bytes": (_int, [_i32, _i32, _i32, _i64p]),
    "ce_fh_decompress": (_int, [_i32, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _i32, C.c_float, _vp]),
    "ce_fh_compress": (_int, [_i32, _vp, _i64, _i64, _i64, _vp, _i64, _i64, _i64, _i64, _i64, _i32, _i32, _i32, _i32, C.c_float, _vp]),
    # PRACH preamble detection: scalars and pointers only, the host view is the transforms' (m_sc holds n_fft)
    "ce_prach_derive_host": (_int, [_i32, _i32, _i32, _P(_i32), _i32, _i32, _i32, _P(TpHostView), _P(_i32), _P(_i32)]),
    "ce_prach_copy_tables": (_int, [_i32, _i32, _i32, _P(_i32), _vp, _vp]),
    "ce_prach_plan_create": (_int, [_i32, _i32, _i32, _i32, _i32, _P(_i32), _i32, _i32, _i32, _P(_vp)]),
    "ce_prach_plan_destroy": (None, [_vp]),
    "ce_prach_detect": (_int, [_vp, _vp, _i64, _i64, _i64, _i64, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    # SRS channel estimation: scalars and pointers only, the host view is the transforms' (m_sc holds n_fft)
    "ce_srs_derive_host": (_int, [_i32] * 7 + [_vp] + [_i32] * 7 + [_vp, _P(TpHostView), _vp, _vp, _vp, _vp, _vp, _vp]),
    "ce_srs_copy_tables": (_int, [_i32] * 6 + [_vp, _vp, _vp]),
    "ce_srs_plan_create": (_int, [_i32] * 9 + [_vp] + [_i32] * 7 + [_vp, _P(_vp)]),
    "ce_srs_plan_destroy": (None, [_vp]),
    "ce_srs_profile": (_int, [_vp, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _vp]),
    "ce_srs_estimate": (_int, [_vp, _vp, _i64, _i64, _i64, _i64, _i32, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
})
CE_FH_NONE, CE_FH_BFP, CE_FH_MAX_PRBS = 0, 1, 341
CE_LDPC_MAX_ZC, CE_LDPC_MAX_ROWS, CE_LDPC_MAX_COLS, CE_LDPC_MAX_ROW_DEGREE = 384, 46, 68, 19
CE_LDPC_L_BOUND, CE_LDPC_LDS_MAX, CE_LDPC_F32, CE_LDPC_I8 = 4497, 163840, 0, 1
CE_LDPC_STATE_IDX_SHIFT, CE_LDPC_STATE_MAG_SHIFT = 19, 24
_i32p = C.POINTER(C.c_int32)


class LdpcDesc(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("device", C.c_int32), ("zc", C.c_int32), ("n_rows", C.c_int32), ("n_cols", C.c_int32),
                ("n_punctured_cols", C.c_int32), ("n_in", C.c_int32), ("k_out", C.c_int32), ("in_format", C.c_int32),
                ("max_iters", C.c_int32), ("early_stop", C.c_int32), ("llr_scale", C.c_float),
                ("row_start", _i32p), ("col", _i32p), ("shift", _i32p)]


class LdpcInfo(C.Structure):
    _fields_ = [("n_edges", C.c_int32), ("row_bytes", C.c_int32), ("n_bits", C.c_int32), ("blocks_per_workgroup", C.c_int32),
                ("threads", C.c_int32), ("lds_bytes", C.c_int32)]


class LdpcHostView(C.Structure):
    _fields_ = [("n_sys", C.c_int32), ("n_edges", C.c_int32), ("max_row_degree", C.c_int32), ("max_col_degree", C.c_int32),
                ("row_bytes", C.c_int32), ("n_bits", C.c_int32), ("threads_per_block", C.c_int32),
                ("blocks_per_workgroup", C.c_int32), ("threads", C.c_int32), ("lds_l_bytes", C.c_int32),
                ("lds_state32_bytes", C.c_int32), ("lds_state8_bytes", C.c_int32), ("lds_bytes_per_block", C.c_int32),
                ("lds_flag_bytes", C.c_int32), ("lds_bytes", C.c_int32), ("schedule_bytes", C.c_int32),
                ("state_idx_shift", C.c_int32), ("state_mag_shift", C.c_int32)]


REGISTRY["ce_ldpc.h"] = Header(structs={"ce_ldpc_desc": LdpcDesc, "ce_ldpc_info": LdpcInfo, "ce_ldpc_host_view": LdpcHostView}, signatures={   # extension
    "ce_ldpc_derive_host": (_int, [_P(LdpcDesc), _P(LdpcHostView)]),
    "ce_ldpc_plan_create": (_int, [_P(LdpcDesc), _P(_vp)]),
    "ce_ldpc_plan_destroy": (None, [_vp]),
    "ce_ldpc_plan_get_info": (_int, [_vp, _P(LdpcInfo)]),
    "ce_ldpc_decode": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp]),
})
CE_TB_G24A, CE_TB_G24B, CE_TB_G16, CE_TB_THREADS, CE_TB_MAX_PIECE = 0x864CFB, 0x800063, 0x1021, 256, 5


class TbDesc(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("device", C.c_int32), ("base_graph", C.c_int32), ("tbs", C.c_int32)]


class TbInfo(C.Structure):
    _fields_ = [("n_code_blocks", C.c_int32), ("in_row_bytes", C.c_int32), ("tb_row_bytes", C.c_int32), ("reserved0", C.c_int32),
                ("bytes_per_slot", C.c_int64)]


class TbHostView(C.Structure):
    _fields_ = [("b", C.c_int32), ("k_cb", C.c_int32), ("c", C.c_int32), ("b_prime", C.c_int32), ("k_prime", C.c_int32),
                ("l_tb", C.c_int32), ("l_cb", C.c_int32), ("p", C.c_int32), ("g_tb", C.c_int32), ("g_cb", C.c_int32),
                ("in_row_bytes", C.c_int32), ("tb_row_bytes", C.c_int32), ("piece_dwords", C.c_int32), ("threads", C.c_int32),
                ("blocks_per_workgroup", C.c_int32), ("lds_bytes", C.c_int32), ("fold_slots_per_workgroup", C.c_int32),
                ("power_bytes", C.c_int32)]


REGISTRY["ce_tb.h"] = Header(structs={"ce_tb_desc": TbDesc, "ce_tb_info": TbInfo, "ce_tb_host_view": TbHostView}, signatures={   # extension
    "ce_tb_derive_host": (_int, [_P(TbDesc), _P(TbHostView)]),
    "ce_tb_plan_create": (_int, [_P(TbDesc), _P(_vp)]),
    "ce_tb_plan_destroy": (None, [_vp]),
    "ce_tb_plan_get_info": (_int, [_vp, _P(TbInfo)]),
    "ce_tb_assemble": (_int, [_vp, _vp, _i64, _vp, _vp, _vp, _vp]),
})
CE_ENC_THREADS, CE_ENC_CORE_TRIANGULAR, CE_ENC_CORE_NR, CE_ENC_CRC_CHUNK = 256, 0, 1, 1024


class EncDesc(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("device", C.c_int32), ("base_graph", C.c_int32), ("tbs", C.c_int32), ("qm", C.c_int32),
                ("n_layers", C.c_int32), ("g_bits", C.c_int32), ("n_ref", C.c_int32), ("n_rows", C.c_int32), ("n_cols", C.c_int32),
                ("row_start", _i32p), ("col", _i32p), ("shift", _i32p)]


class EncInfo(C.Structure):
    _fields_ = [("n_code_blocks", C.c_int32), ("tb_row_bytes", C.c_int32), ("g_row_bytes", C.c_int32), ("cw_row_bytes", C.c_int32),
                ("cw_required", C.c_int32), ("reserved0", C.c_int32), ("bytes_per_slot", C.c_int64)]


class EncHostView(C.Structure):
    _fields_ = [("b", C.c_int32), ("k_cb", C.c_int32), ("c", C.c_int32), ("b_prime", C.c_int32), ("k_prime", C.c_int32),
                ("k_b", C.c_int32), ("zc", C.c_int32), ("k", C.c_int32), ("n", C.c_int32), ("n_cb", C.c_int32),
                ("f0", C.c_int32), ("f1", C.c_int32), ("p_rm", C.c_int32), ("n_lo", C.c_int32), ("e_lo", C.c_int32),
                ("e_hi", C.c_int32), ("k0", C.c_int32 * 4), ("s", C.c_int32 * 4), ("l_tb", C.c_int32), ("l_cb", C.c_int32),
                ("p", C.c_int32), ("g_tb", C.c_int32), ("g_cb", C.c_int32), ("tb_row_bytes", C.c_int32), ("g_row_bytes", C.c_int32),
                ("cw_row_bytes", C.c_int32), ("n_sys", C.c_int32), ("n_edges", C.c_int32), ("core_form", C.c_int32),
                ("core_rows", C.c_int32), ("core_shift", C.c_int32), ("rows_needed", C.c_int32), ("col_dwords", C.c_int32),
                ("ext_dwords", C.c_int32), ("cw_required", C.c_int32), ("threads", C.c_int32), ("lds_bytes", C.c_int32),
                ("table_bytes", C.c_int32)]


REGISTRY["ce_enc.h"] = Header(structs={"ce_enc_desc": EncDesc, "ce_enc_info": EncInfo, "ce_enc_host_view": EncHostView}, signatures={   # extension
    "ce_enc_derive_host": (_int, [_P(EncDesc), _P(EncHostView)]),
    "ce_enc_plan_create": (_int, [_P(EncDesc), _P(_vp)]),
    "ce_enc_plan_destroy": (None, [_vp]),
    "ce_enc_plan_get_info": (_int, [_vp, _P(EncInfo)]),
    "ce_enc_encode": (_int, [_vp, _vp, _vp, _i64, _i64, _vp, _vp, _vp]),
})
CE_MAX_LAYERS, CE_MOD_THREADS, CE_MOD_TILE_SC, CE_MOD_GROUP_SYMBOLS, CE_MOD_MAX_TILE_BLOCKS = 4, 256, 256, 7, 34
CE_MOD_A_QPSK, CE_MOD_A_16QAM, CE_MOD_A_64QAM, CE_MOD_A_256QAM = 0x3F3504F3, 0x3EA1E89B, 0x3E1E01B3, 0x3D9D130E
CE_MOD_A = {2: CE_MOD_A_QPSK, 4: CE_MOD_A_16QAM, 6: CE_MOD_A_64QAM, 8: CE_MOD_A_256QAM}   # float32 bit patterns of A_qm


class ModHopDesc(C.Structure):
    _fields_ = [("dmrs_symbols", C.c_uint8 * CE_MAX_SYMBOLS), ("re_mask", C.c_uint16 * CE_MAX_CDM), ("reserved_re_mask", C.c_uint16),
                ("prb_start", C.c_int32), ("n_prbs", C.c_int32), ("start_symbol", C.c_int32), ("n_alloc_symbols", C.c_int32),
                ("mask_prbs", C.POINTER(C.c_uint8))]


class ModDesc(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("device", C.c_int32), ("n_prb_grid", C.c_int32), ("n_sym", C.c_int32), ("n_layers", C.c_int32),
                ("qm", C.c_int32), ("scramble", C.c_int32), ("n_hops", C.c_int32), ("hop", ModHopDesc * CE_MAX_HOPS)]


class ModInfo(C.Structure):
    _fields_ = [("n_bits", C.c_int32), ("n_symbols", C.c_int32), ("n_data_re", C.c_int32), ("g_row_bytes", C.c_int32), ("n_re", C.c_int32),
                ("n_dmrs_total", C.c_int32), ("bytes_per_slot", C.c_int64)]


class ModHostView(C.Structure):
    _fields_ = [("n_bits", C.c_int32), ("g_row_bytes", C.c_int32), ("n_data_re", C.c_int32), ("n_symbols", C.c_int32), ("n_re", C.c_int32),
                ("n_dmrs_total", C.c_int32), ("sym_hop", C.c_int32 * CE_MAX_SYMBOLS), ("data_mask", C.c_int32 * CE_MAX_SYMBOLS),
                ("data_res_per_prb", C.c_int32 * CE_MAX_SYMBOLS), ("first_row", C.c_int32 * CE_MAX_SYMBOLS),
                ("dmrs_col", C.c_int32 * CE_MAX_SYMBOLS), ("n_words", C.c_int32), ("block_words", C.c_int32), ("n_blocks", C.c_int32),
                ("table_bytes", C.c_int32), ("tile_sc", C.c_int32), ("tiles_per_symbol", C.c_int32), ("group_symbols", C.c_int32), ("n_groups", C.c_int32),
                ("workgroups_per_slot", C.c_int32),
                ("max_tile_blocks", C.c_int32), ("threads", C.c_int32), ("lds_bytes", C.c_int32)]


REGISTRY["ce_mod.h"] = Header(structs={"ce_mod_hop_desc": ModHopDesc, "ce_mod_desc": ModDesc, "ce_mod_info": ModInfo, "ce_mod_host_view": ModHostView}, signatures={   # extension
    "ce_mod_derive_host": (_int, [_P(ModDesc), _P(ModHostView)]),
    "ce_mod_plan_create": (_int, [_P(ModDesc), _P(_vp)]),
    "ce_mod_plan_destroy": (None, [_vp]),
    "ce_mod_plan_get_info": (_int, [_vp, _P(ModInfo)]),
    "ce_mod_modulate": (_int, [_vp, _vp, _vp, _i64, C.c_float, _vp, _vp, _i64p, _i64, _vp, _vp]),
})
EXPORTS, EXPORTS_DENOISE = list(REGISTRY["ce_hip.h"].signatures), list(REGISTRY["ce_denoise.h"].signatures)
ALL_EXPORTS = [name for header in REGISTRY.values() for name in header.signatures]


# per-source compiler flags: the denoiser's MFMA results feed vector instructions straight away, so keep them in
# VGPRs (the default AGPR form costs four v_accvgpr_read per 16x16 tile in a kernel bound by vector-instruction issue)
EXTRA_FLAGS = {"ce_denoise.hip": ["-mllvm", "-amdgpu-mfma-vgpr-form"],
               # wide single-hop FIR kernels (the headline's among them): max-ILP scheduling, 2-3 % faster in process; the narrow tiers lose with it
               "ce_inst_reg_h1_f1w.hip": ["-mllvm", "-amdgpu-sched-strategy=max-ilp"],
               # the wave-per-item kernel is bound by vector-instruction issue: the SLP vectoriser's packed-f32 forms cost a register
               # move or two per packed operation there (850 v_mov in one kernel against 465 without) -- in process 10-18 % faster on
               # the one-layer two-hop shapes without it, 0-4 % on the multi-layer ones (profiles/round3_narrow_kernel_ab.txt)
               "ce_inst_narrow.hip": ["-fno-slp-vectorize"],
               # the same for the two-hop and the re-read units (in process, all units without it: two-hop wide tiers -1...-4 %, 2 hops x 40
               # PRB -7 %, iterated in-painting -5 %, 4 layers x 2 hops -2 %; the one-hop register units are indifferent and keep the default;
               # profiles/round3_noslp_ab.txt)
               "ce_inst_reg_h2_f0.hip": ["-fno-slp-vectorize"], "ce_inst_reg_h2_f1.hip": ["-fno-slp-vectorize"],
               "ce_inst_gen_h2.hip": ["-fno-slp-vectorize"],
               # the one-hop re-read unit also without the loop vectoriser (its staged writer's store loop otherwise pairs iterations into
               # v_pk_mul/fma_f32 at ~50 register moves per 8 stores): 2 / 4 layers at full band -1 ... -2 % in two in-process A/Bs, bit-identical;
               # the two-hop unit measured +2 % with it and keeps the vectoriser (profiles/round3_reread_batched_loads_ab.txt)
               "ce_inst_gen_h1.hip": ["-fno-slp-vectorize", "-fno-vectorize"]}


def build(force: bool = False, verbose: bool = False, extra_flags=(), out: Path | None = None) -> Path:
    """hipcc --offload-arch=gfx950 -> csrc/libce_hip.so (cross-compiles without a GPU): one object per source
    (compiled concurrently, each with its own flags), then one link."""
    from concurrent.futures import ThreadPoolExecutor

    srcs = [CSRC / s for s in SOURCES]
    deps = build_deps()
    shipped = CSRC / "libce_hip.so"                         # build() always writes the in-tree library, whatever CE_HIP_LIB selects for loading
    target = Path(out) if out is not None else shipped
    if out is None and not force and all(t.exists() and all(t.stat().st_mtime >= d.stat().st_mtime for d in deps) for t in (shipped, KNOBS_LIB_PATH)):
        return shipped
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    objdir = CSRC / ".build" if out is None else Path(str(target) + ".obj")   # diagnostic builds (tools/) keep their own objects
    objdir.mkdir(exist_ok=True)
    common = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{INCLUDE}", f"-I{CSRC}", *extra_flags]

    def compile_one(src: Path) -> Path:
        obj = objdir / (src.stem + ".o")
        cmd = common + EXTRA_FLAGS.get(src.name, []) + ["-c", str(src), "-o", str(obj)]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True)
        return obj

    def compile_knobs() -> Path:                               # ce_api.hip is the only unit that looks at the knobs
        obj = objdir / "ce_api_knobs.o"
        cmd = common + ["-DCE_TUNING_KNOBS=1", "-c", str(CSRC / "ce_api.hip"), "-o", str(obj)]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True)
        return obj

    with ThreadPoolExecutor(max_workers=min(len(srcs) + 1, os.cpu_count() or 4)) as pool:
        knobs_obj = pool.submit(compile_knobs) if out is None else None
        objs = list(pool.map(compile_one, srcs))
        knobs_obj = knobs_obj.result() if knobs_obj is not None else None

    def link(objects, dst):
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(dst)] + [str(o) for o in objects]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True)

    link(objs, target)
    if knobs_obj is not None:
        link([knobs_obj if o.name == "ce_api.o" else o for o in objs], KNOBS_LIB_PATH)
    return target


_lib = None


def load() -> C.CDLL:
    """Load the HIP library; raise loudly when it is absent (no fallback path exists)."""
    global _lib
    if _lib is not None:
        return _lib
    if not LIB_PATH.exists():
        raise RuntimeError(f"{LIB_PATH} is not built: run `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(the estimator has no CPU fallback)")
    lib = C.CDLL(str(LIB_PATH))
    for header in REGISTRY.values():
        for name, (restype, argtypes) in header.signatures.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    if lib.ce_abi_version() != CE_ABI_VERSION:
        raise RuntimeError(f"libce_hip.so ABI {lib.ce_abi_version()} != binding {CE_ABI_VERSION}; rebuild")
    _lib = lib
    return lib


def last_error() -> str:
    return load().ce_last_error().decode("utf-8", "replace")
