"""The workgroup -> work-item map (`item_of` in ce_estimate_kernel.h) and the store order it gives the grid writers,
checked on the CPU: the map is compiled for the host from the kernel header itself and enumerated.

* every batch shape: each item is written by exactly one workgroup (a permutation), full blocks and ragged tail alike;
* a slot's Rx ports land on workgroups 8 apart (one XCD, one L2), and each XCD's slots form one contiguous range;
* the direct writers' iterations, for every symbol / layer geometry they serve, visit every 16-byte chunk of an item once."""
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CSRC = ROOT / "srsran_ce_pytorch_amd" / "csrc"

_PROG = r"""
#include "ce_estimate_kernel.h"
#include <cstdio>
#include <cstdlib>
int main(int argc, char** argv) {
  for (int a = 1; a + 1 < argc; a += 2) {
    const int n_ports = atoi(argv[a]);
    const long n_items = atol(argv[a + 1]);
    for (long b = 0; b < n_items; ++b) printf("%ld ", (long)item_of(b, n_ports, n_items));
    printf("\n");
  }
  return 0;
}
"""

SHAPES = [(1, 1), (4, 2), (4, 4), (32, 4), (68, 4), (8192 * 4, 4), (1024, 1), (1030, 1), (40, 2), (15, 3), (27, 3), (240, 3),
          (128 * 5 + 5, 5), (7 * 8, 8), (64 * 8 + 16, 8), (2048 * 2 + 6, 2)]


@pytest.fixture(scope="module")
def item_maps(tmp_path_factory):
    d = tmp_path_factory.mktemp("item_of")
    (d / "item_of.hip").write_text(_PROG)
    exe = d / "item_of"
    subprocess.run(["hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "--cuda-host-only", f"-I{ROOT / 'include'}", f"-I{CSRC}",
                    str(d / "item_of.hip"), "-o", str(exe)], check=True, capture_output=True)
    args = [str(x) for n_items, n_ports in SHAPES for x in (n_ports, n_items)]
    lines = subprocess.run([str(exe), *args], check=True, capture_output=True, text=True).stdout.splitlines()
    return {shape: [int(x) for x in line.split()] for shape, line in zip(SHAPES, lines)}


@pytest.mark.parametrize("n_items,n_ports", SHAPES)
def test_item_map_is_a_permutation_with_xcd_local_slots(item_maps, n_items, n_ports):
    m = item_maps[(n_items, n_ports)]
    assert sorted(m) == list(range(n_items))
    per = 8 * n_ports
    full = n_items // per * per
    assert m[full:] == list(range(full, n_items)), "ragged tail: identity"
    wg_of = {item: b for b, item in enumerate(m)}
    xcd_slots = {x: [] for x in range(8)}
    for slot in range(full // n_ports):
        wgs = [wg_of[slot * n_ports + p] for p in range(n_ports)]
        assert len({b % 8 for b in wgs}) == 1, f"slot {slot}: ports on workgroups {wgs}"
        xcd_slots[wgs[0] % 8].append(slot)
    n_blocks = n_items // per
    for x, slots in xcd_slots.items():
        assert slots == list(range(x * n_blocks, (x + 1) * n_blocks)), f"XCD {x}: its slots are not one contiguous eighth"


@pytest.mark.parametrize("ns2", [7, 6])     # 14- / 12-symbol slots
@pytest.mark.parametrize("L", [1, 3])       # the direct (whole-PRB step) writers
def test_direct_writer_visits_every_chunk_once(ns2, L):
    """write_grid_direct / write_grid_direct_ovl: thread tid < ACTIVE owns phase tid % ROW4 of subcarrier tid / ROW4 and
    stores at tid + it * ACTIVE for it < ceil((n_sc - sc_lane) / SC_STEP): every float4 of the item exactly once, at 273 PRB
    (91 iterations of 4032 bytes for one layer and 14 symbols) and every other grid width."""
    NT = 256
    ROW4 = ns2 * L
    ACTIVE = (NT // (36 * ns2)) * (36 * ns2)
    SC_STEP = ACTIVE // ROW4
    assert SC_STEP % 12 == 0
    for n_prb in (1, 3, 11, 25, 52, 106, 272, 273):
        n_sc = 12 * n_prb
        hits = [0] * (n_sc * ROW4)
        for tid in range(ACTIVE):
            sc_lane = tid // ROW4
            n_iter = (n_sc - sc_lane + SC_STEP - 1) // SC_STEP
            for it in range(n_iter):
                hits[tid + it * ACTIVE] += 1
        assert hits == [1] * len(hits), f"{n_prb} PRB"
        if (n_prb, ns2, L) == (273, 7, 1):
            assert (ACTIVE * 16, -(-n_sc // SC_STEP)) == (4032, 91)
