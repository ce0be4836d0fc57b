"""The combine-and-deliver route (``spartan_amd.array.combine``) on a real
MI355X: the case table of tests/test_combine.py through the real backend,
every result compared with NumPy value by value (integers below 2^53: exact in
any order), plus a NaN and a tie that cross tiles.
"""
import numpy as np
import pytest

from test_combine import HINTS, OPS, _case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('W', [1, 4])
@pytest.mark.parametrize('op', OPS)
def test_case_table_gpu(gpu_workers, op, W):
  gpu_workers(W)
  for hint in HINTS:
    build, want = _case(op, hint)
    np.testing.assert_array_equal(build().glom(), want, err_msg=str(hint))


@pytest.mark.parametrize('W', [1, 4])
def test_min_keeps_a_nan_of_one_tile(gpu_workers, W):
  from spartan_amd import expr
  gpu_workers(W)
  nf = np.arange(1200.).reshape(40, 30)
  nf[37, 4] = np.nan  # in the last row block: merged into the columns' minimum after three finite blocks
  for hint in HINTS:
    x = expr.from_numpy(nf, tile_hint=hint).force()
    got = expr.min(x, 0).glom()
    assert np.isnan(got[4])
    np.testing.assert_array_equal(got, nf.min(0), err_msg=str(hint))


@pytest.mark.parametrize('W', [1, 4])
def test_argmax_tie_across_tiles_takes_the_first(gpu_workers, W):
  from spartan_amd import expr
  gpu_workers(W)
  nt = np.arange(1200.).reshape(40, 30) % 7
  nt[5, 3] = nt[25, 3] = 99.  # rows 5 and 25: different tiles under every row cut
  nt[25, 20] = 99.            # a later column of the same value: axis None keeps (5, 3)
  for hint in HINTS:
    x = expr.from_numpy(nt, tile_hint=hint).force()
    assert int(expr.argmax(x, 0).glom()[3]) == 5
    assert int(expr.argmax(x).glom()) == 5 * 30 + 3
    for axis in (None, 0, 1):
      np.testing.assert_array_equal(expr.argmax(x, axis).glom(), nt.argmax(axis), err_msg='%s %s' % (hint, axis))
