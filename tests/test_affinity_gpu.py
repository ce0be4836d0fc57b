"""spx_pairwise, ``expr.pairwise_kernel`` / ``expr.normalized_affinity`` and the
spectral-clustering driver on a real MI355X, at the sizes where
the kernel can go wrong: n and m one less than, exactly and one more than the
tile edge TB and at 2 TB + 3 (two tiles and a rest), n != m among them; d at 1,
one less than, exactly and one more than the k-chunk KC and at 130 (nine
chunks, the last partial).  TB and KC are read from the plan.  Leading
dimensions larger than the row (column slices of wider tensors, 16-byte aligned
and not), out only / row sums only / both, scales with a diagonal at a non-zero
first column, forced splits, empty calls.

The yardstick is affinity_ref.pairwise_ref -- the formulas evaluated literally
in float64 on the same, already rounded, inputs -- with the derived bound
``|got - ref| <= TOL (1 + gamma s) |ref| + tiny`` of that module (TOL 1e-5 /
1e-12; tests/test_affinity.py shows plain float32 arithmetic inside it for
these very inputs), summed over the row for the degrees and doubled for L.
The exactness properties are asserted bit for bit.
"""
import functools

import numpy as np
import pytest

from affinity_ref import (METRICS, affinity_ref, assert_degrees_within, assert_within, blobs, edge_shapes, from_sums,
                          gamma_for, pair_sums, points, same_partition)

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


def _plan(dtype=np.float32):
  from spartan_amd import binding
  return binding.pairwise_plan(dtype, 1, 1)[:2]  # (TB, KC)


def _dev(a):
  import torch
  return torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared inputs are read-only)


@functools.lru_cache(maxsize=None)
def _case(n, m, d, dtype):
  """(X, Y, s, l1) of one case, computed once and shared (never written).  Row
  1 of Y is row 2 of X where both exist: an identical pair in every case."""
  X, Y = points(n, d, dtype, 3), points(m, d, dtype, 4)
  if n > 2 and m > 1:
    Y[1] = X[2]
  s, l1 = pair_sums(X, Y)
  for arr in (X, Y, s, l1):
    arr.setflags(write=False)
  return X, Y, s, l1


def _pairwise(X, Y, metric, gamma, **kw):
  from spartan_amd import backend
  return backend.get().pairwise(X, Y, metric, gamma, **kw)


# ---------------------------------------------------------------- spx_pairwise
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('metric', METRICS)
def test_edge_shapes_against_yardstick(gpu_ctx, metric, dtype):
  tb, kc = _plan(dtype)
  worst = 0.0
  for n, m, d in edge_shapes(tb, kc):
    X, Y, s, l1 = _case(n, m, d, dtype)
    gamma = gamma_for(d)
    ref, gs = from_sums(s, l1, metric, gamma)
    out, sums = _pairwise(_dev(X), _dev(Y), metric, gamma, out=True, row_sums=True)
    what = (metric, np.dtype(dtype).name, n, m, d)
    assert out.shape == (n, m) and sums.shape == (n,) and out.dtype == sums.dtype == _dev(X).dtype
    got = out.cpu().numpy()
    worst = max(worst, assert_within(got, ref, gs, dtype, what))
    assert_degrees_within(sums.cpu().numpy(), ref, gs, dtype, what)
    assert got[2, 1] == (1.0 if metric == 'rbf' else 0.0), what  # identical rows: exact
  print('%s %s: max error / bound = %.3g' % (metric, np.dtype(dtype).name, worst))


@pytest.mark.parametrize('dtype', DTYPES)
def test_out_only_sums_only_and_both_agree(gpu_ctx, dtype):
  import torch
  tb, kc = _plan(dtype)
  n, m, d = tb + 1, 2 * tb + 3, kc + 1
  X, Y, s, l1 = _case(n, m, d, dtype)
  x, y = _dev(X), _dev(Y)
  for metric in METRICS:
    both = _pairwise(x, y, metric, gamma_for(d), out=True, row_sums=True)
    only_out = _pairwise(x, y, metric, gamma_for(d), out=True)
    only_sums = _pairwise(x, y, metric, gamma_for(d), row_sums=True)
    assert only_out[1] is None and only_sums[0] is None
    assert torch.equal(only_out[0], both[0]) and torch.equal(only_sums[1], both[1]), metric
    # tensors to fill are filled in place and returned
    o = torch.full((n, m), -1.0, dtype=x.dtype, device='cuda')
    r = torch.full((n,), -1.0, dtype=x.dtype, device='cuda')
    got = _pairwise(x, y, metric, gamma_for(d), out=o, row_sums=r)
    assert got[0] is o and got[1] is r and torch.equal(o, both[0]) and torch.equal(r, both[1])


@pytest.mark.parametrize('dtype', DTYPES)
def test_leading_dimensions_larger_than_the_row(gpu_ctx, dtype):
  """Column slices of wider tensors: at a 16-byte aligned offset with aligned
  rows (the vector loads and stores) and at an odd offset (the scalar ones);
  out a slice too.  The wider tensors' other columns stay as they were."""
  import torch
  tb, kc = _plan(dtype)
  n, m = tb + 1, 2 * tb + 3
  for d in (kc, kc + 1):
    X, Y, s, l1 = _case(n, m, d, dtype)
    ref, gs = from_sums(s, l1, 'rbf', gamma_for(d))
    plain = _pairwise(_dev(X), _dev(Y), 'rbf', gamma_for(d), out=True)[0]
    for off, pad in ((4, 8), (3, 5)):
      wx = torch.full((n, d + pad), 7.0, dtype=plain.dtype, device='cuda')
      wy = torch.full((m, d + pad), 7.0, dtype=plain.dtype, device='cuda')
      wo = torch.full((n, m + pad), 7.0, dtype=plain.dtype, device='cuda')
      wx[:, off:off + d] = _dev(X)
      wy[:, off:off + d] = _dev(Y)
      out, sums = _pairwise(wx[:, off:off + d], wy[:, off:off + d], 'rbf', gamma_for(d), out=wo[:, off:off + m],
                            row_sums=True)
      assert out.stride(0) == m + pad
      assert torch.equal(out, plain), (d, off)  # the same bits as the contiguous call
      assert_within(out.cpu().numpy(), ref, gs, dtype, ('ld', d, off))
      assert_degrees_within(sums.cpu().numpy(), ref, gs, dtype, ('ld', d, off))
      assert bool((wo[:, :off] == 7.0).all()) and bool((wo[:, off + m:] == 7.0).all())


@pytest.mark.parametrize('dtype', DTYPES)
def test_scales_and_a_diagonal_at_a_nonzero_first_column(gpu_ctx, dtype):
  """A row slab of the scaled pass: rows lo .. lo + n of the m points against
  all of them, scaled by r_i c_j, the slab's own diagonal (column lo + i)
  overridden in out but not in the row sums."""
  tb, kc = _plan(dtype)
  m, d, lo = 2 * tb + 3, kc + 1, tb - 3
  n = tb + 1  # the slab crosses a tile edge, and so does its diagonal
  Y = points(m, d, dtype, 5)
  X = Y[lo:lo + n]
  r = np.random.RandomState(6)
  rs, cs = r.uniform(0.5, 2.0, n).astype(dtype), r.uniform(0.5, 2.0, m).astype(dtype)
  for metric in ('rbf', 'euclidean'):
    a, gs = from_sums(*pair_sums(X, Y), metric, gamma_for(d))
    scale = rs.astype(np.float64)[:, None] * cs.astype(np.float64)[None, :]
    ref = a * scale
    out, sums = _pairwise(_dev(X), _dev(Y), metric, gamma_for(d), out=True, row_sums=True, row_scale=_dev(rs),
                          col_scale=_dev(cs), diag_col0=lo, diag_value=-3.0)
    got = out.cpu().numpy()
    i = np.arange(n)
    assert np.all(got[i, lo + i] == -3.0), metric
    want = ref.copy()
    want[i, lo + i] = -3.0
    # one more rounding a scale product and a scaling: the factor 2 of L's bound
    assert_within(got, want, gs, dtype, ('scaled', metric), factor=2.0)
    assert_degrees_within(sums.cpu().numpy(), ref, gs, dtype, ('scaled sums', metric))
    # without an override the diagonal holds the computed value
    plain = _pairwise(_dev(X), _dev(Y), metric, gamma_for(d), out=True, row_scale=_dev(rs), col_scale=_dev(cs))[0]
    keep = np.ones((n, m), bool)
    keep[i, lo + i] = False
    assert np.array_equal(plain.cpu().numpy()[keep], got[keep]) and not np.any(plain.cpu().numpy()[i, lo + i] == -3.0)


@pytest.mark.parametrize('dtype', DTYPES)
def test_forced_splits(gpu_ctx, dtype):
  """1, 2 and 3 column ranges: out does not depend on the split at all; the row
  sums are inside the bound for each split, and the same split gives the same
  bits again."""
  import torch
  from spartan_amd import binding
  tb, kc = _plan(dtype)
  n, m, d = tb + 1, 2 * tb + 3, kc - 1
  X, Y, s, l1 = _case(n, m, d, dtype)
  ref, gs = from_sums(s, l1, 'rbf', gamma_for(d))
  outs, sums = [], []
  for splits in (1, 2, 3):
    assert binding.pairwise_plan(dtype, n, m, splits)[2] == splits
    o, r = _pairwise(_dev(X), _dev(Y), 'rbf', gamma_for(d), out=True, row_sums=True, splits=splits)
    assert_degrees_within(r.cpu().numpy(), ref, gs, dtype, ('splits', splits))
    outs.append(o)
    sums.append(r)
    again = _pairwise(_dev(X), _dev(Y), 'rbf', gamma_for(d), row_sums=True, splits=splits)[1]
    assert torch.equal(again, r), splits  # the same split: the same bits
  assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])
  # more splits than column tiles: the trailing ranges are empty and add exact zeros
  o, r = _pairwise(_dev(X), _dev(Y), 'rbf', gamma_for(d), out=True, row_sums=True, splits=7)
  assert torch.equal(o, outs[0])
  assert_degrees_within(r.cpu().numpy(), ref, gs, dtype, ('splits', 7))


def test_empty_calls(gpu_ctx):
  import torch
  X = torch.zeros((5, 3), dtype=torch.float32, device='cuda')
  none = torch.zeros((0, 3), dtype=torch.float32, device='cuda')
  out, sums = _pairwise(none, X, 'rbf', 1.0, out=True, row_sums=True)
  assert out.shape == (0, 5) and sums.shape == (0,)
  out, sums = _pairwise(X, none, 'rbf', 1.0, out=True, row_sums=True)
  assert out.shape == (5, 0) and torch.equal(sums, torch.zeros_like(sums))


# ------------------------------------------------------------------ exactness
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('metric', METRICS)
def test_duplicates_symmetry_and_reruns_are_exact(gpu_ctx, metric, dtype):
  import torch
  tb, kc = _plan(dtype)
  n, d = 2 * tb + 3, kc + 1
  P = points(n, d, dtype, 8)
  P[tb + 2] = P[5]  # duplicates in different tiles
  P[tb - 1] = P[5]
  x = _dev(P)
  same = 1.0 if metric == 'rbf' else 0.0
  A, D = _pairwise(x, x, metric, gamma_for(d), out=True, row_sums=True)
  assert torch.equal(A, A.T)
  assert bool((torch.diagonal(A) == same).all()) and float(A[5, tb + 2]) == same and float(A[tb - 1, tb + 2]) == same
  A2, D2 = _pairwise(x, x, metric, gamma_for(d), out=True, row_sums=True)
  assert torch.equal(A, A2) and torch.equal(D, D2)
  assert torch.equal(D[5], D[tb + 2])  # identical points have identical rows, so identical degrees
  # the scaled pass keeps the symmetry: the product of the two scales is formed first
  sc = _dev(np.random.RandomState(9).uniform(0.1, 3.0, n).astype(dtype))
  L = _pairwise(x, x, metric, gamma_for(d), out=True, row_scale=sc, col_scale=sc, diag_col0=0, diag_value=1.0)[0]
  assert torch.equal(L, L.T) and bool((torch.diagonal(L) == 1.0).all())


@pytest.mark.parametrize('dtype', DTYPES)
def test_nan_poisons_its_own_row_and_column_only_and_huge_gamma_is_zero(gpu_ctx, dtype):
  import torch
  tb, kc = _plan(dtype)
  n, d = tb + 5, kc + 1
  P = points(n, d, dtype, 10)
  P[7, kc] = np.nan  # in the partial second chunk
  x = _dev(P)
  mask = torch.zeros((n, n), dtype=torch.bool, device='cuda')
  mask[7, :] = True
  mask[:, 7] = True
  for metric in METRICS:
    A = _pairwise(x, x, metric, gamma_for(d), out=True)[0]
    assert torch.equal(torch.isnan(A), mask), metric
  Q = _dev(points(n, d, dtype, 11))
  A = _pairwise(Q, Q, 'rbf', 1e30, out=True)[0]
  assert torch.equal(A, torch.eye(n, dtype=A.dtype, device='cuda'))  # exp(-huge) = 0, exp(-0) = 1


# ------------------------------------------------------------- expression layer
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('W', [1, 2, 3])
def test_expr_layouts_on_the_device(gpu_workers, W, dtype):
  gpu_workers(W)
  from spartan_amd import expr
  tb, kc = _plan(dtype)
  n, m, d = 2 * tb + 3, tb + 1, kc + 1
  X, Y, s, l1 = _case(n, m, d, dtype)
  gamma = gamma_for(d)
  ref, gs = from_sums(s, l1, 'rbf', gamma)
  L_ref, D_ref, A_ref, gsx = affinity_ref(X, 'rbf', gamma, 1.0)
  first = None
  for hint in ((n, d), (50, d), (tb, d)):  # one slab; 50 50 31; 64 64 3
    x = expr.from_numpy(X, tile_hint=hint)
    K = expr.pairwise_kernel(x, expr.from_numpy(Y, tile_hint=(40, d)), metric='rbf', gamma=gamma)
    got = K.glom()
    assert got.dtype == np.dtype(dtype)
    assert_within(got, ref, gs, dtype, ('pairwise_kernel', W, hint))
    cuts = sorted({(e.ul[0], e.lr[0]) for e in x.force().tiles})
    assert sorted((e.ul, e.lr) for e in K.force().tiles) == [((lo, 0), (hi, m)) for lo, hi in cuts]
    Kxx = expr.pairwise_kernel(x, metric='manhattan').glom()
    assert np.array_equal(Kxx, Kxx.T) and np.all(np.diag(Kxx) == 0)
    L, D = expr.normalized_affinity(x, metric='rbf', gamma=gamma)
    got_L, got_D = L.glom(), D.glom()
    assert got_L.dtype == got_D.dtype == np.dtype(dtype)
    assert_degrees_within(got_D, A_ref, gsx, dtype, ('D', W, hint))
    assert_within(got_L, L_ref, gsx, dtype, ('L', W, hint), factor=2.0)
    assert np.array_equal(got_L, got_L.T) and np.all(np.diag(got_L) == 1.0)
    assert sorted((e.ul, e.lr) for e in L.force().tiles) == [((lo, 0), (hi, n)) for lo, hi in cuts]
    if first is None:
      first = (got_L, got_D)
    # a row's values do not depend on the slab it is computed in
    assert np.array_equal(got_L, first[0]) and np.array_equal(got_D, first[1]), hint


# ---------------------------------------------------------------------- driver
@pytest.mark.parametrize('dtype', DTYPES)
def test_driver_on_the_device(gpu_workers, dtype):
  gpu_workers(2)
  from spartan_amd import expr
  from spartan_amd.examples.spectral_clustering import spectral_cluster
  pts, truth = blobs(90, 2, 3, dtype=dtype)
  labels = spectral_cluster(expr.from_numpy(pts, tile_hint=(32, 2)), k=3, num_iter=5)
  got = labels.glom().reshape(-1)
  assert got.shape == (90,) and same_partition(got, truth)
