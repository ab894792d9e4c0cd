"""The structure cases of tests/structure_cases.py -- saturated class lists, full residual lists, placed intra macroblocks, heights around the
deblocking groups -- through the kernels' source built for the host (tests/emu) against the oracle: every variant of tests/test_layouts_emu.py on
the tight layout, one padded layout on one variant.  Every picture's census is asserted where its packets are made (structure_cases.packets).
The host build runs the waves one after another: it holds the list logic, the bitmap and the group geometry, not the order in which the device
runs them (tests/test_hip_structure.py)."""
import pytest

from tests import structure_cases as S
from tests.test_layouts_emu import VARIANTS, libs, run_case  # noqa: F401 (libs: the fixture)

GEOMS = [(c[0], w, h) for c in S.SATURATED + S.PLACED for (w, h) in c[1]]


def run(libs, oracle, variant, layout, name, w, h):
    pkts = S.packets(name, w, h)
    _, _, pattern, kw, _ = S.CASES[name]
    run_case(libs, variant, layout, w, h, pattern, kw, S.seed_of(name, w, h), oracle=oracle, name=name, packets=[p for p, _ in pkts])


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("name,w,h", GEOMS, ids=[f"{n}_{w}x{h}" for n, w, h in GEOMS])
def test_structure_emu_vs_oracle(libs, oracle, name, w, h, variant):
    run(libs, oracle, variant, "tight", name, w, h)


@pytest.mark.parametrize("name,w,h", GEOMS, ids=[f"{n}_{w}x{h}" for n, w, h in GEOMS])
def test_structure_on_a_padded_layout(libs, oracle, name, w, h):
    run(libs, oracle, list(VARIANTS)[(len(name) + h) % len(VARIANTS)], "pad16", name, w, h)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("height", S.TAIL_HEIGHTS)
def test_tail_heights_emu_vs_oracle(libs, oracle, height, variant):
    """luma groups of 8 rows, chroma groups of 15: chroma heights that are whole groups, tails of one row, a luma tail beside a full chroma group"""
    for w in S.TAIL_WIDTHS:
        run(libs, oracle, variant, "tight", "tails", w, height)


@pytest.mark.parametrize("height", S.TAIL_HEIGHTS)
def test_tail_heights_on_a_padded_layout(libs, oracle, height):
    for k, w in enumerate(S.TAIL_WIDTHS):
        run(libs, oracle, list(VARIANTS)[(k + height) % len(VARIANTS)], "pad16", "tails", w, height)
