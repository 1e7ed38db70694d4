"""What a kernel *variant* is, and a bounded sweep of slot descriptors that reaches every variant the shipped selection
policy can pick (ce_api.hip: select_kernel).

The estimator runs one of many compiled template instances (csrc/ce_inst_*.hip), each with run-time branches that change
its LDS layout and stage order.  A bug in one of them shows up only on the shapes that select it, so the suite derives its
cases from the policy instead of listing them by hand: ``sweep()`` walks the descriptors, ``ce_plan_derive_host`` reports
what each one selects, and ``representatives()`` keeps the first descriptor per selection tuple as a seeded
``synth.case_spec``.  When the policy moves, the representatives move with it.

Used by tests/test_kernel_variants.py (CPU: coverage and instance census) and tests/test_hip_kernel_variants.py (GPU:
each representative against the float64 oracle).  A plain module, not a conftest."""
from __future__ import annotations

import ctypes as C
import re
from functools import lru_cache

import numpy as np

from srsran_ce_pytorch_amd import _lib, estimator as E, synth as S

GRIDS = (52, 106, 273)
N_SYMS = (14, 13, 12)
SMOOTHINGS = ("none", "mean", "filter", "mmse")
INTERPS = ("linear", "cnn")
LAYERS = (1, 2, 3, 4)
ALL_RE = [1] * 12
# DM-RS RE masks: one CDM group for 1-2 layers, two for 3-4 (every RE a pilot: one group only)
MASKS = {"type1": ([S.TYPE1_CDM0], [S.TYPE1_CDM0, S.TYPE1_CDM1]),
         "type2": ([S.TYPE2_CDM0], [S.TYPE2_CDM0, S.TYPE2_CDM1]),
         "allre": ([ALL_RE], None)}
PER_PRB = {"type1": 6, "type2": 4, "allre": 12}
# Pilots per DM-RS symbol at which the policy changes its mind (csrc/ce_plan.h, ce_api.hip: select_kernel):
# 24 one-hop one-layer narrow kernel (CE_NARROW_1H1L_MAX_RE), 192 narrow kernel (CE_NARROW_MAX_RE), 256 / 512 / 1024 register
# tiers KPT 1 / 2 / 4 (CE_THREADS), 1728 windowed RC FIR ((CE_THREADS - 64) * CE_CONV_C), 1792 widest register tier (CE_KPT * CE_THREADS)
RE_BOUNDS = (24, 192, 256, 512, 1024, 1728, 1792)
# the standard bands: one to three PRB (short RC filters), the reference harness's 25 / 52, 50 of 106, 100, full 273
STANDARD_PRBS = (1, 2, 3, 25, 50, 52, 100, 106, 273)


def prb_counts(mask: str, grid: int):
    """Both sides of every pilot-count boundary for this mask (the last PRB count at or below it and the first above),
    plus the standard bands and the full grid -- each in the smallest swept grid that holds it (a band selects the same
    kernel in any grid; the small grid keeps the oracle cheap)."""
    n = set(STANDARD_PRBS) | {grid}
    for t in RE_BOUNDS:
        n.update((t // PER_PRB[mask], t // PER_PRB[mask] + 1))
    smaller = max([g for g in GRIDS if g < grid], default=0)
    return sorted(x for x in n if smaller < x <= grid or x == grid)


def _dmrs_lists(n_sym: int):
    """DM-RS symbol lists by count: one hop over the slot, and the two halves of a hopping slot (valid in 12-14 symbols)."""
    h = n_sym // 2
    one = {1: [2], 2: [2, 9], 3: [2, 6, 9], 4: [1, 4, 7, 10], 5: [1, 3, 5, 7, 9]}
    first = {1: [2], 2: [0, 3], 3: [0, 2, 4], 4: [0, 1, 3, 5]}
    return one, first, {k: [h + s for s in v] for k, v in first.items()}, h


def hops_of(grid, mask, layers, n_prb, pos, layout, nd, n_sym):
    """``synth.hop_spec`` list of one sweep point.  ``layout``: "one" (one hop, the band at the lower / upper grid edge by
    ``pos``), or two hops -- the first at the lower, the second at the upper edge -- over the two halves of the slot
    ("split"), over ranges that share two symbols ("partial"), or both over the whole slot ("full").  ``nd`` is the DM-RS
    count per hop, or (hop 1, hop 2)."""
    re_masks = MASKS[mask][0 if layers <= 2 else 1]
    one, first, second, h = _dmrs_lists(n_sym)
    top = grid - n_prb
    if layout == "one":
        return [S.hop_spec(one[nd], 0 if pos == "lo" else top, n_prb, 0, n_sym, re_masks)]
    nd1, nd2 = nd if isinstance(nd, tuple) else (nd, nd)
    rng = {"split": ((0, h), (h, n_sym - h)), "partial": ((0, h + 2), (h - 2, n_sym - h + 2)), "full": ((0, n_sym), (0, n_sym))}[layout]
    return [S.hop_spec(first[nd1], 0, n_prb, rng[0][0], rng[0][1], re_masks),
            S.hop_spec(second[nd2], top, n_prb, rng[1][0], rng[1][1], re_masks)]


# The standard shapes, first in the sweep so that each stays a representative whatever else reaches its tuple:
# (grid, mask, layers, n_prb, pos, layout, nd, smoothing, interp, n_sym)
NAMED = {
    "52prb_full_band": (52, "type1", 1, 52, "lo", "one", 2, "filter", "linear", 14),
    "50_of_106": (106, "type1", 1, 50, "lo", "one", 2, "filter", "linear", 14),
    "2x50_of_106": (106, "type1", 1, 50, "lo", "split", 2, "filter", "linear", 14),
    **{f"tier_{t}_last_{t // 6}prb": (273, "type1", 1, t // 6, "lo", "one", 2, "filter", "linear", 14) for t in (256, 512, 1024)},
    **{f"tier_{t}_first_{t // 6 + 1}prb": (273, "type1", 1, t // 6 + 1, "lo", "one", 2, "filter", "linear", 14) for t in (256, 512, 1024)},
    **{f"tier_{t}_last_{t // 12}prb_allre": (273, "allre", 1, t // 12, "lo", "one", 2, "filter", "linear", 14) for t in (256, 512, 1024)},
    **{f"tier_{t}_first_{t // 12 + 1}prb_allre": (273, "allre", 1, t // 12 + 1, "lo", "one", 2, "filter", "linear", 14) for t in (256, 512, 1024)},
}


def sweep():
    """Every sweep point, deterministic order, named shapes first."""
    yield from NAMED.values()
    for grid in GRIDS:
        for mask in MASKS:
            for layers in LAYERS:
                if MASKS[mask][0 if layers <= 2 else 1] is None:
                    continue
                for n_prb in prb_counts(mask, grid):
                    geos = [("lo", "one", nd) for nd in (1, 2, 3, 4, 5)]
                    if n_prb < grid:                    # the upper band edge (the second hop of a two-hop point sits there too)
                        geos += [("hi", "one", 2)]
                    geos += [("lo", lay, nd) for lay in ("split", "partial", "full") for nd in (1, 2, 3, 4, (2, 1))]
                    for pos, layout, nd in geos:
                        for n_sym in N_SYMS:
                            for smoothing in SMOOTHINGS:
                                for interp in INTERPS:
                                    # "mean" selects what "none" selects (same feature set and LDS): swept on 14-symbol linear points only
                                    if smoothing != "mean" or (n_sym == 14 and interp == "linear"):
                                        yield (grid, mask, layers, n_prb, pos, layout, nd, smoothing, interp, n_sym)


def case_of(point, name: str, seed: int):
    """A sweep point as a seeded ``synth.case_spec`` (+ its interpolator): noise on every RE, a CFO and a delay (the
    synth defaults), CFO compensation where the grid has the 14 symbols it needs."""
    grid, mask, layers, n_prb, pos, layout, nd, smoothing, interp, n_sym = point
    case = S.case_spec(name, grid, hops_of(grid, mask, layers, n_prb, pos, layout, nd, n_sym), n_layers=layers,
                       smoothing=smoothing, cfo_compensate=n_sym == 14, n_sym=n_sym, seed=seed)
    return case, interp


# --------------------------------------------------------------------------------------------------------------------
# Host derivation of one point, without the estimator's Python validation (the sweep makes some 10^5 of them)
# --------------------------------------------------------------------------------------------------------------------
_SM = _lib.SMOOTHING
_MMSE_TAU_NSR = (float(S.normal_cp_ms(30e3)[1]) * 1e-3, 0.01)   # estimator._resolve's defaults for Smoothing="mmse"


@lru_cache(maxsize=None)
def _prb_mask(grid, start, n):
    m = np.zeros(grid, np.uint8)
    m[start:start + n] = 1
    return (C.c_uint8 * grid).from_buffer_copy(m.tobytes())


def _mask_bits(col):
    return sum(1 << r for r in range(12) if col[r])


def derive_point(point):
    """``ce_plan_derive_host`` of a sweep point, or None where the library refuses it (e.g. mmse smoothing of a mask
    whose pilot spacing differs between blocks)."""
    grid, mask, layers, n_prb, pos, layout, nd, smoothing, interp, n_sym = point
    hops = hops_of(grid, mask, layers, n_prb, pos, layout, nd, n_sym)
    d = _lib.PlanDesc()
    d.abi_version, d.device, d.n_prb_grid, d.n_sym, d.n_layers, d.n_hops = _lib.CE_ABI_VERSION, 0, grid, n_sym, layers, len(hops)
    d.smoothing, d.cfo_compensate, d.interp = _SM[smoothing], int(n_sym == 14), _lib.INTERP[interp]
    d.scs_hz, d.beta_dmrs = 30e3, 1.4125
    d.mmse_delay_spread_s, d.mmse_noise_to_signal = _MMSE_TAU_NSR
    d.cp_ms[:] = S.normal_cp_ms(30e3).tolist()
    for i, h in enumerate(hops):
        hd = d.hop[i]
        for s in h["dmrs_symbols"]:
            hd.dmrs_symbols[s] = 1
        for c, col in enumerate(h["re_masks"]):
            hd.re_mask[c] = _mask_bits(col)
        hd.prb_start, hd.n_prbs = h["prb_start"], h["n_prbs"]
        hd.mask_prbs = C.cast(_prb_mask(grid, h["prb_start"], h["n_prbs"]), C.POINTER(C.c_uint8))
        hd.start_symbol, hd.n_alloc_symbols = h["start_symbol"], h["n_alloc"]
    v = _lib.PlanHostView()
    return v if _lib.load().ce_plan_derive_host(C.byref(d), C.byref(v)) == 0 else None


def derive_case(case, interp):
    """``ce_plan_derive_host`` of a case, through the estimator's own descriptor path (what a GPU test's plan derives)."""
    hop1, hop2, cfg = S.numpy_hops(case)
    return E.derive_host(hop1, hop2, cfg, case["beta"], case["n_layers"], case["n_prb_grid"], case["n_sym"], interp)


# --------------------------------------------------------------------------------------------------------------------
# The selection tuple
# --------------------------------------------------------------------------------------------------------------------
def instance_of(view):
    """The compiled instance a launch runs: (instantiation unit source, key of the unit's switch)."""
    return _lib.KERNEL_UNITS[view.kernel_unit], int(view.kernel_key)


def variant_of(view, n_sym: int, interp: str):
    """The selection tuple of a derived plan: the instance plus every run-time branch that changes LDS layout, stage
    order or writer.  Layers and hops come from the instance key / unit (what the launch really uses).

    Wave-per-item kernel: (narrow, layers, hops, n_sym class, interp form, filter).  Added to the issue's definition:
    ``filter`` -- the kernel's RC-filter stage has its own halo layout (nrw_halo); interp form instead of the interpolator
    -- see below.

    Workgroup kernels: (hops, feat, layers, reg_nd, reg_kpt or "rr" (re-read), ta_lp, ta_over_p, pil_stash class,
    sym_overlap, filt_windowed where the smoothing is the RC filter, n_sym class, interp form, smoothing where feat == 3).
    Added: the interp form -- linear, or ce_dl_cnn's in-painting in its comb-2 closed form (cnn_comb2 1), binomial closed
    form in the staged writer (2) or iterated (0): three writers of their own; and for the extension feature set the
    smoothing, since mmse (MFMA block filter) and the iterated in-painting with or without the RC filter are separate stages
    of the same instance.  Dropped: nothing.  Not distinguished: none vs mean (one reduction apart), CNNSmoothingAlpha."""
    unit, key = instance_of(view)
    ns = n_sym if n_sym in (12, 14) else "other"
    form = "lin" if interp == "linear" else f"cnn{int(view.cnn_comb2)}"
    if unit == "ce_inst_narrow.hip":
        return ("narrow", key // 10, key % 10, ns, form, "f" if view.rc_len > 0 else "-")
    hops = 2 if "_h2" in unit else 1
    feat, layers = key // 10000, key // 1000 % 10
    nd, kpt = int(view.reg_nd), ("rr" if view.reg_nd == 0 else int(view.reg_kpt))
    stash = "none" if view.pil_stash == 0 else ("all" if (view.pil_stash >> 24) == nd else "partial")
    smoothing = "filter" if view.rc_len > 0 else ("mmse" if view.mmse_w[0][0][0] != 0.0 else "nm")
    return ("wg", hops, feat, layers, nd, kpt, int(view.ta_lp), int(view.ta_over_p), stash, int(view.sym_overlap),
            int(view.filt_windowed) if smoothing == "filter" else "-", ns, form, smoothing if feat == 3 else "-")


def variant_id(t) -> str:
    """A test id for a tuple."""
    if t[0] == "narrow":
        return f"narrow-L{t[1]}-h{t[2]}-s{t[3]}-{t[4]}-{'filt' if t[5] == 'f' else 'nofilt'}"
    _, hops, feat, layers, nd, kpt, lp, op, stash, ov, win, ns, form, sm = t
    return (f"h{hops}-f{feat}-L{layers}-nd{nd}-k{kpt}-lp{lp}-op{op}-st{stash}-ov{ov}-w{win}-s{ns}-{form}"
            + (f"-{sm}" if sm != "-" else ""))


@lru_cache(maxsize=None)
def census():
    """Walk the sweep once: ``(first point per tuple, set of instances reached, number of points derived)``."""
    first, instances, n = {}, set(), 0
    for point in sweep():
        v = derive_point(point)
        if v is None:
            continue
        n += 1
        instances.add(instance_of(v))
        first.setdefault(variant_of(v, point[9], point[8]), point)
    return first, frozenset(instances), n


def representatives():
    """``[(test id, tuple, case_spec, interp)]``: the first sweep point of every reachable tuple as a seeded case, plus every
    named standard shape (a named shape whose tuple an earlier one already holds is kept under its own name)."""
    first, _, _ = census()
    out, seen = [], set()
    for i, (t, point) in enumerate(first.items()):
        case, interp = case_of(point, variant_id(t), seed=1000 + i)
        out.append((variant_id(t), t, case, interp))
        seen.add(point)
    for i, (name, point) in enumerate(NAMED.items()):
        if point not in seen:
            v = derive_point(point)
            t = variant_of(v, point[9], point[8])
            case, interp = case_of(point, name, seed=5000 + i)
            out.append((f"{variant_id(t)}[{name}]", t, case, interp))
    return out


# --------------------------------------------------------------------------------------------------------------------
# What is compiled: the instantiation units read as source
# --------------------------------------------------------------------------------------------------------------------
def _kpt_wide() -> int:
    src = (_lib.CSRC / "ce_plan.h").read_text()
    threads = int(re.search(r"#define CE_THREADS (\d+)", src).group(1))
    return 7 if threads == 256 else 4                   # CE_KPT (ce_plan.h)


def _active_lines(text: str, defines: dict):
    """The lines of a unit body that survive its #if / #ifdef / #ifndef / #else / #endif under ``defines`` (integer macros;
    ``#define NAME <int>`` in an active region adds one).  Enough for ce_inst.inc; anything else is an error."""
    stack, out = [], []
    for line in text.replace("\\\n", " ").splitlines():
        s = line.strip()
        active = all(stack)
        if s.startswith("#if "):
            expr = s[4:].split("//")[0]
            stack.append(active and bool(eval(re.sub(r"\b[A-Z_][A-Z0-9_]*\b", lambda m: str(defines[m.group(0)]), expr))))
        elif s.startswith("#ifndef "):
            stack.append(active and s.split()[1] not in defines)
        elif s.startswith("#ifdef "):
            stack.append(active and s.split()[1] in defines)
        elif s.startswith("#else"):
            stack[-1] = all(stack[:-1]) and not stack[-1]
        elif s.startswith("#endif"):
            stack.pop()
        elif active and s.startswith("#define "):
            m = re.match(r"#define (\w+) (-?\d+)\b", s)
            if m:
                defines[m.group(1)] = int(m.group(2))
        elif active and not s.startswith("#"):
            out.append(line.split("//")[0])
    assert not stack, "unbalanced conditionals"
    return out


def compiled_instances():
    """Every (unit source, key) the instantiation units compile: ce_inst.inc expanded for each ce_inst_*.hip that
    includes it, and the switch of ce_inst_narrow.hip."""
    kpt = _kpt_wide()
    inst = set()
    for unit in _lib.SOURCES:
        if not unit.startswith("ce_inst_"):
            continue
        src = (_lib.CSRC / unit).read_text()
        defines = {k: int(v) for k, v in re.findall(r"#define (CE_TU_\w+) (-?\d+)", src)}
        body = "\n".join(_active_lines((_lib.CSRC / "ce_inst.inc").read_text(), dict(defines))) if '#include "ce_inst.inc"' in src \
            else "\n".join(_active_lines(src, {}))
        val = lambda x: kpt if x.strip() == "CE_KPT" else int(x)   # noqa: E731
        for a in re.findall(r"\bCE_NRW\(([^)]*)\)", body):
            L, nh = map(val, a.split(","))
            inst.add((unit, L * 10 + nh))
        for macro, args in re.findall(r"\b(CE_REG|CE_CASE|CE_GEN)\(([^)]*)\)", body):
            a = [x.strip() for x in args.split(",")]
            if macro == "CE_REG":                       # CE_CASE(CE_TU_FEAT, 1, ND, KC, KT)
                a = [str(defines["CE_TU_FEAT"]), "1"] + a
            if macro == "CE_GEN":                       # CE_CASE(F, L, 0, 0, CE_KPT) for L = 1..4
                for L in (1, 2, 3, 4):
                    inst.add((unit, val(a[0]) * 10000 + L * 1000))
                continue
            f, L, nd, kc = (val(x) for x in a[:4])
            inst.add((unit, f * 10000 + L * 1000 + nd * 10 + kc))
    return inst
