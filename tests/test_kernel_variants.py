"""CPU-only checks of the kernel-variant census (tests/kernel_variants.py) against the shipped library: every compiled
instance is reachable by the selection policy, every representative still selects its own tuple, and the representatives
cover every reachable tuple -- so tests/test_hip_kernel_variants.py runs every variant the policy can pick."""
import numpy as np
import pytest

import kernel_variants as K
from srsran_ce_pytorch_amd import _lib


@pytest.fixture(scope="module", autouse=True)
def lib():
    _lib.build()
    return _lib.load()


def test_compiled_instances_are_the_reachable_ones():
    """The (unit, key) pairs the instantiation units compile equal those the sweep reaches: a dead instantiation, or a
    policy change that strands one, fails here."""
    compiled = K.compiled_instances()
    _, reached, n_points = K.census()
    assert n_points > 10000
    assert compiled - reached == set(), f"compiled but never selected: {sorted(compiled - reached)}"
    assert reached - compiled == set(), f"selected but not compiled: {sorted(reached - compiled)}"
    assert len(compiled) == 95


def test_representatives_cover_every_reachable_tuple():
    first, _, _ = K.census()
    reps = K.representatives()
    assert {t for _, t, _, _ in reps} == set(first)
    ids = [vid for vid, _, _, _ in reps]
    assert len(set(ids)) == len(ids), "test ids must be unique"
    named = {case["name"] for _, _, case, _ in reps} | {K.variant_id(t) for t, point in first.items() if point in K.NAMED.values()}
    for name, point in K.NAMED.items():                  # each standard shape is a representative, under its tuple or its name
        assert name in named or first[K.variant_of(K.derive_point(point), point[9], point[8])] == point, name


def test_representatives_select_their_own_tuple():
    """Through the estimator's own descriptor path -- what the GPU test's plan derives."""
    wrong = []
    for vid, t, case, interp in K.representatives():
        v = K.derive_case(case, interp)
        if K.variant_of(v, case["n_sym"], interp) != t:
            wrong.append(vid)
    assert not wrong, wrong[:10]


def test_representatives_are_well_conditioned_inputs():
    """Noise on every RE, a CFO, a delay, and more than 2 pilots per symbol (time alignment is unpinned at 2 or fewer)."""
    for vid, _, case, interp in K.representatives():
        assert case["noise_var"] > 0 and case["cfo_hz"] != 0 and case["delay_ns"] != 0, vid
        v = K.derive_case(case, interp)
        assert v.n_re > 2, vid


def test_standard_shapes_select_the_expected_instances():
    """The issue's mid-band shapes, by name: 52 PRB full band and 50 of 106 (filter, 2 DM-RS, one layer) run the one-hop
    KPT-2 filter instance; two hops of 50 PRB the two-hop one with both hops' transforms side by side."""
    def inst(name):
        point = K.NAMED[name]
        v = K.derive_point(point)
        return K.instance_of(v), int(v.ta_lp)
    assert inst("52prb_full_band") == (("ce_inst_reg_h1_f1.hip", 11022), 1)
    assert inst("50_of_106") == (("ce_inst_reg_h1_f1.hip", 11022), 1)
    assert inst("2x50_of_106") == (("ce_inst_reg_h2_f1.hip", 11022), 2)
    kpts = [K.derive_point(K.NAMED[n]).reg_kpt for n in ("tier_256_last_42prb", "tier_256_first_43prb", "tier_512_last_85prb",
                                                         "tier_512_first_86prb", "tier_1024_last_170prb", "tier_1024_first_171prb")]
    assert kpts == [1, 2, 2, 4, 4, 7]


def test_instance_census_reads_the_units():
    """The unit reader against two hand-counted facts: 15 cases per register unit pair / re-read h1 unit, 8 narrow."""
    inst = K.compiled_instances()
    per_unit = {u: sum(1 for x, _ in inst if x == u) for u in _lib.KERNEL_UNITS}
    assert per_unit == {"ce_inst_narrow.hip": 8, "ce_inst_reg_h1_f0.hip": 15, "ce_inst_reg_h1_f1.hip": 8,
                        "ce_inst_reg_h1_f1w.hip": 7, "ce_inst_reg_h2_f0.hip": 15, "ce_inst_reg_h2_f1.hip": 15,
                        "ce_inst_gen_h1.hip": 15, "ce_inst_gen_h2.hip": 12}
    assert np.all([k > 0 for _, k in inst])
