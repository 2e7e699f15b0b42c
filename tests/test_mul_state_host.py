"""The reference of the Mul state (tests/mul_state_ref.py) checked against itself and the oracle, on the exact inputs of
tests/test_gpu_mul_state.py -- no GPU.

(1) The bound holds for the model it was derived from, and is exercised: the model's rows differ from the exact ones.
(2) The bound discriminates: with the lo plane dropped (model B), or a view's part summed in float32 (model C), every row that at
    least half of the views touch exceeds 100 (B[c] + B[k]) in some class.  A condition on the inputs: a case that misses it gets a
    longer run or larger triangles, never a lower factor.  Where every contributing pixel is folded on its own (the texel cases) a
    fold's part is a single float32 term: there is no sum for model C to get wrong, and only model B is asked for.
(3) The reference's get() agrees with the oracle's float64 accumulators at 1e-6.

Smallest ratio error / (B[c] + B[k]) over those rows, of the row maximum (model B / model C): a19 3.5e5 / 4.1e4, a7 1.1e5 / 3.1e4,
a48 4.3e5 / 6.9e4, b19 3.4e5 / 1.1e5, c19 4.7e5 / 1.3e5, d64 1.1e6 / 6.1e5, d150 1.3e6 / 4.7e5, d520 1.5e6 / 5.2e5,
f19 2.9e5 / 6.2e4, g19 2.9e5 / 1.2e5, sparse19 1.8e5 / 3.1e5, n5 1.3e5 / 7.6e4 (without its two rows that end with no finite pair
to compare), e5 6.8e4, e5big 8.1e4; the model itself stays below 0.04 of the bound.
"""
import functools

import numpy as np
import pytest

import mul_state_ref as R

FACTOR = 100.0
DISCRIMINATING = list(R.BOUND_CASES)


@functools.lru_cache(maxsize=None)
def run(name):
    cs = R.case(name)
    ref = R.MulReference(cs.P, cs.C, cs.iew, cs.fold_per, broken=True)
    for i in range(cs.views):
        k, probs, weights = R.view_inputs(cs, i)
        ref.add(cs.planes[k], probs, weights)
    return cs, ref


def row_ratio(ref, values):
    """Per row, the largest error / (B[c] + B[k]) over its finite elements."""
    err, pb = ref.centred_error(values), ref.pair_bound()
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(np.isfinite(err) & (pb > 0), err / pb, 0.0)
    return q.max(axis=1)


@pytest.mark.parametrize("name", R.BOUND_CASES)
def test_bound_holds_for_the_model(name):
    cs, ref = run(name)
    model = ref.hi + ref.lo
    assert R.same_class(model, ref.exact64())
    err, pb = ref.centred_error(model), ref.pair_bound()
    fin = np.isfinite(err)
    assert fin.any() and (err[fin] <= pb[fin]).all()
    differ = int((np.where(fin, err, 0.0).max(axis=1) > 0).sum())
    print("%s: model error / bound at most %.3g; rows that differ from the exact ones: %d" % (name, row_ratio(ref, model).max(), differ))
    assert differ >= 10                                                # the bound is exercised, not a test for == 0


@pytest.mark.parametrize("name", DISCRIMINATING)
def test_bound_discriminates(name):
    cs, ref = run(name)
    rows = ref.views_touched * 2 >= cs.views
    if name == "n5":                                                   # two of its rows end without a finite pair to compare
        rows[[R.nonfinite_rows()["emptied"], R.nonfinite_rows()["infinite"]]] = False
    assert rows.sum() >= 100
    b = row_ratio(ref, ref.hi_b)[rows].min()
    c = row_ratio(ref, ref.hi_c + ref.lo_c)[rows].min()
    print("%s: %d rows; smallest ratio without lo %.3g, with float32 parts %.3g" % (name, int(rows.sum()), b, c))
    assert b > FACTOR
    if cs.fold_per == "view":
        assert c > FACTOR


def test_nonfinite_members_of_the_reference():
    """Case n5's edits land: the classes they name, and only those, are not finite at the end of the run."""
    cs, ref = run("n5")
    e, rows = ref.exact64(), R.nonfinite_rows()
    assert np.isneginf(e[rows["wiped"]]).tolist() == [False, False, True, False, False]
    assert np.isneginf(e[rows["emptied"]]).all() and not ref.get()[rows["emptied"]].any()
    assert np.isnan(e[rows["negative"]]).tolist() == [False, True, False, False, False]
    assert np.isposinf(e[rows["infinite"]]).tolist() == [True, False, False, False, False]
    assert np.isfinite(e[rows["unweighted"]]).all()
    others = np.ones(cs.P, bool)
    others[list(rows.values())] = False
    assert np.isfinite(e[others]).all()


def test_reference_pinned_to_the_oracle(oracle):
    """Sixteen views of case a19: the reference's get() against OracleAggregator("mul") with float64 accumulators."""
    cs = R.case("a19")
    ref = R.MulReference(cs.P, cs.C, cs.iew)
    oracle.set_accum_double(True)
    try:
        oagg = oracle.OracleAggregator(cs.P, cs.C, "mul", cs.iew)
        for i in range(16):
            k, probs, weights = R.view_inputs(cs, i)
            ref.add(cs.planes[k], probs, weights)
            oagg.add(cs.planes[k], probs, weights)
        want = oagg.get()
    finally:
        oracle.set_accum_double(False)
    assert (ref.views_touched > 0).sum() > cs.P // 2
    np.testing.assert_allclose(ref.get(), want, rtol=1e-6, atol=1e-35)       # (atol: float32 denormals of the oracle's result)
