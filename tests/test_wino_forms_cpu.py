"""The table of point-GEMM forms (convops.WINO_FORMS) against what the forms are elsewhere - no GPU, no build. Per form:
  the FLOP meter's count for a synthetic argument tuple = 2 x 16 x R x Cout x Cin x (K loops of Cin per output plane: the depth taps, 2, 3/2),
  the weight shape and the operand rows = what the plain-torch restatements (wino_cases.py, wino_dn_cases.py, wino_dn4_cases.py) produce for
  n = 1, D = 8, Ht = Wt = 8, C = 32, Cout = 32,
  every entry the row names is one of the C ABI.
"""
import math
from fractions import Fraction

import pytest
import torch

import wino_cases as wc
import wino_dn4_cases as d4
import wino_dn_cases as dn
from forge_amd import _lib, convops as co, flopmeter as fm

N, D, HT, WT, C, COUT = 1, 8, 8, 8, 32, 32
LOOPS = {"points": 3, "half": 3, "dn": 2, "dn4": Fraction(3, 2)}                     # K loops of Cin per output plane, three depth taps
WEIGHTS = {"points": lambda wp: wc.weights(wp, 3), "half": lambda wp: wc.weights(wp, 3), "dn": dn.weights_dn, "dn4": d4.weights_dn4}
OPERAND = {"points": wc.input_transform, "half": wc.input_transform, "dn": wc.input_transform, "dn4": d4.input_transform_dn4}


def test_the_table_lists_the_four_forms():
    assert sorted(co.WINO_FORMS) == sorted(LOOPS)
    assert {k: f.P for k, f in co.WINO_FORMS.items()} == {"points": 16, "half": 8, "dn": 16, "dn4": 16}


@pytest.mark.parametrize("name", sorted(LOOPS))
def test_flop_meter_counts_the_forms_k_loops(name):
    form = co.WINO_FORMS[name]
    n, Dd, C1, C2, Cout = 2, 32, 128, 128, 256
    args = [None, C1, C1, 0, 0, None, C2, C2, 0, 0, None, None, n, Dd, 16, 16, Cout, 3] + ([0] if name == "points" else []) + [None]
    R = n * Dd * 16 * 16
    assert fm._ENTRIES[form.gemm](args) == float(2 * 16 * R * Cout * (C1 + C2) * LOOPS[name])


@pytest.mark.parametrize("name", sorted(LOOPS))
def test_shapes_are_the_restatements(name):
    form = co.WINO_FORMS[name]
    g = torch.Generator().manual_seed(20)
    U = WEIGHTS[name](torch.randn(27, COUT, C, generator=g))
    shape = form.ushape(3, COUT, C)
    # the restatements keep the entries' own layout [16][positions][Cout][Cin]; the F(2, 3) nest's tensor splits its four positions as [2][2]
    assert shape[0] == 16 and shape[-2:] == (COUT, C) and math.prod(shape[1:-2]) == U.shape[1] and math.prod(shape) == U.numel(), (shape, U.shape)
    V = OPERAND[name](torch.randn(N, D, 2 * HT, 2 * WT, C, generator=g))
    assert V.shape == (16, N * D * HT * WT * form.rows, C), (V.shape, form.rows)


@pytest.mark.parametrize("name", sorted(LOOPS))
def test_entries_are_of_the_c_abi(name):
    form = co.WINO_FORMS[name]
    assert {form.gemm, form.weights, form.input} <= set(_lib.SIGNATURES)
