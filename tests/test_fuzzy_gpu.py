"""spx_fuzzy_step, the fuzzy expression layer and the fuzzy k-means driver on a
real MI355X, at the sizes where the kernel can go wrong: one
row and one centre; fewer rows, centres and columns than any tile; centre
counts on both sides of the 64-centre blocks the waves share (3, 17, 64, 65,
256); D below, at and above a column panel (128 float32 / 64 float64 columns:
33, 128 and 130 take the ragged, the whole and the chunked path); and N =
2 row_tile groups + 3, where every group walks more than one row tile and the
last sub-tile is ragged.  In the first six shapes row 3 of X IS centre 0: at
m = 1.1 (exponent 20) a plain d^-e overflows there (1e-11^-20), so that case
shows the dmin normalisation.

The yardstick is fuzzy_ref.fuzzy_ref -- the K^2 form evaluated literally in
float64 on the same, already rounded, inputs.  Tolerances are the project's
parity tolerances: U absolute 1e-5 (float32) / 1e-12 (float64); counts and sums
relative to the array's largest magnitude, the same two numbers.  Labels are
exact; the test first asserts that the yardstick's two smallest distances of
every row differ by more than 1e-5 relative, so rounding cannot swap them.
"""
import functools

import numpy as np
import pytest

from fuzzy_ref import SHAPES, fuzzy_blobs, fuzzy_data, fuzzy_kmeans_loop, fuzzy_ref, top_two_gap

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
TOL = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-12}
EPS = 1e-11
SEED = 7
MID = (300, 33, 17, 2.0)


def _dev(a):
  import torch
  return torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared inputs are read-only)


def _host(t):
  return None if t is None else t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(shape, dtype, seed=SEED, weight_power=1.0, blobs=False):
  """(X, C, yardstick) of one shape, computed once and shared (never written)."""
  n, d, k, m = shape
  X, C = (fuzzy_blobs if blobs else fuzzy_data)(n, d, k, dtype, seed)
  ref = fuzzy_ref(X, C, 2.0 / (m - 1.0), EPS, weight_power)
  for a in (X, C) + tuple(ref.values()):
    a.setflags(write=False)
  return X, C, ref


def _step(X, C, m, weight_power=1.0, want_labels=True, want_U=True, sums=None, counts=None):
  from spartan_amd import backend
  x = X if not isinstance(X, np.ndarray) else _dev(X)
  return backend.get().fuzzy_step(x, _dev(np.asarray(C, np.float64)), 2.0 / (m - 1.0), EPS, weight_power,
                                  want_labels, want_U, sums=sums, counts=counts)


def _check(what, dtype, ref, labels=None, U=None, sums=None, counts=None):
  tol = TOL[np.dtype(dtype)]
  if labels is not None:
    gap = top_two_gap(ref['dist'])
    print('%s: top-two distance gap %.3g' % (what, gap))
    assert gap > 1e-5, what  # (a seed that violates this is changed; no row is skipped)
    assert labels.dtype == np.int64 and np.array_equal(labels, ref['labels']), what
  if U is not None:
    err = float(np.abs(U.astype(np.float64) - ref['U']).max())
    print('%s: max |dU| %.3g (tolerance %.3g)' % (what, err, tol))
    assert U.dtype == np.dtype(dtype) and err <= tol, what
  for name, got in (('counts', counts), ('sums', sums)):
    if got is not None:
      scale = float(np.abs(ref[name]).max())
      err = float(np.abs(got - ref[name]).max()) / scale
      print('%s: %s relative error %.3g (tolerance %.3g)' % (what, name, err, tol))
      assert got.dtype == np.float64 and got.shape == ref[name].shape and err <= tol, what


# --------------------------------------------------------------- spx_fuzzy_step
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(str(v) for v in s))
def test_step_against_yardstick(gpu_ctx, shape, dtype):
  X, C, ref = _case(shape, dtype)
  if shape[0] > 3:
    assert ref['labels'][3] == 0 and ref['dist'][3, 0] == EPS  # the planted row: its distance is eps alone
  labels, U, sums, counts = (_host(t) for t in _step(X, C, shape[3]))
  assert np.all(np.isfinite(U)) and np.all(np.isfinite(sums)) and np.all(np.isfinite(counts))
  _check('%s %s' % (shape, np.dtype(dtype)), dtype, ref, labels, U, sums, counts)


@pytest.mark.parametrize('dtype', DTYPES)
def test_many_row_tiles_per_group(gpu_ctx, dtype):
  """N = 2 row_tile groups + 3: every group sees two row tiles, one a third, and
  the last sub-tile has three rows.  The points are blobs around the centres:
  among this many plain Gaussian rows some always hold a near tie of the two
  nearest centres (top-two gap 1e-7 .. 4e-6 over eleven seeds), which the label
  check does not allow."""
  from spartan_amd import backend
  row_tile, groups, _kmax, _ws = backend.fuzzy_plan(dtype, 1, 8, 4)
  shape = (2 * row_tile * groups + 3, 8, 4, 2.0)
  X, C, ref = _case(shape, dtype, blobs=True)
  labels, U, sums, counts = (_host(t) for t in _step(X, C, 2.0))
  _check('%s %s' % (shape, np.dtype(dtype)), dtype, ref, labels, U, sums, counts)


@pytest.mark.parametrize('dtype', DTYPES)
def test_strides_and_offsets(gpu_ctx, dtype):
  """ldp > D (a column slice of a wider tensor) and a base one element off any
  16-byte boundary give the results of the contiguous input."""
  import torch
  n, d, k, m = MID
  X, C, ref = _case(MID, dtype)
  wide = torch.zeros((n, d + 7), dtype=_dev(X).dtype, device='cuda')
  wide[:, 3:3 + d] = _dev(X)
  view = wide[:, 3:3 + d]
  assert view.stride(0) == d + 7 and not view.is_contiguous()
  labels, U, sums, counts = (_host(t) for t in _step(view, C, m))
  _check('ldp > D %s' % np.dtype(dtype), dtype, ref, labels, U, sums, counts)
  flat = torch.zeros((n * d + 1,), dtype=wide.dtype, device='cuda')
  flat[1:] = _dev(X).reshape(-1)
  off = flat[1:].view(n, d)
  assert off.data_ptr() % 16 == off.element_size()
  labels, U, sums, counts = (_host(t) for t in _step(off, C, m))
  _check('offset base %s' % np.dtype(dtype), dtype, ref, labels, U, sums, counts)


@pytest.mark.parametrize('dtype', DTYPES)
def test_accumulate_null_outputs_weight_power_and_bits(gpu_ctx, dtype):
  import torch
  n, d, k, m = MID
  X, C, ref = _case(MID, dtype)
  # added on top of what is there
  prior_s = np.random.RandomState(1).randn(k, d)
  prior_c = np.random.RandomState(2).rand(k) + 1.0
  s, c = _dev(prior_s), _dev(prior_c)
  _l, _u, s2, c2 = _step(X, C, m, sums=s, counts=c)
  assert s2 is s and c2 is c
  want = {'sums': prior_s + ref['sums'], 'counts': prior_c + ref['counts']}
  _check('zero_first off %s' % np.dtype(dtype), dtype, want, sums=_host(s), counts=_host(c))
  # null labels / U in every combination: the other outputs are the same bits
  full = [_host(t) for t in _step(X, C, m)]
  for want_labels, want_U in ((True, False), (False, True), (False, False)):
    got = [_host(t) for t in _step(X, C, m, want_labels=want_labels, want_U=want_U)]
    assert (got[0] is None) == (not want_labels) and (got[1] is None) == (not want_U)
    for a, b in zip(full, got):
      assert b is None or a.tobytes() == b.tobytes()
  # a second identical call: byte-identical results
  again = [_host(t) for t in _step(X, C, m)]
  assert all(a.tobytes() == b.tobytes() for a, b in zip(full, again))
  # weight_power = 2, and a fractional one (the general power)
  for wp in (2.0, 1.5):
    _X, _C, ref_w = _case(MID, dtype, SEED, wp)
    labels, U, sums, counts = (_host(t) for t in _step(X, C, m, weight_power=wp))
    _check('weight_power %g %s' % (wp, np.dtype(dtype)), dtype, ref_w, labels, U, sums, counts)


def test_k_above_kmax_is_refused(gpu_ctx):
  from spartan_amd import backend
  kmax = backend.fuzzy_plan(np.float32, 4, 4, 1)[2]
  X, C = fuzzy_data(4, 4, kmax + 1, np.float32)
  with pytest.raises(NotImplementedError, match='kmax = %d' % kmax):
    _step(X, C, 2.0)


# ------------------------------------------------------------------ expr layer
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('hint', [(64, 33), (300, 16)])
def test_expr_layer_on_the_device(gpu_workers, dtype, hint):
  gpu_workers(2)
  from spartan_amd import expr
  n, d, k, m = MID
  X, C, ref = _case(MID, dtype)
  x = expr.from_numpy(X, tile_hint=hint)
  labels, counts, sums = expr.fuzzy_assign(x, C, m=m)
  _check('fuzzy_assign %s %s' % (hint, np.dtype(dtype)), dtype, ref, labels.glom(), None, sums.glom(), counts.glom())
  U = expr.fuzzy_membership(x, C, m=m).glom()
  _check('fuzzy_membership %s %s' % (hint, np.dtype(dtype)), dtype, ref, U=U)


@pytest.mark.parametrize('dtype', DTYPES)
def test_driver_on_the_device(gpu_workers, dtype):
  gpu_workers(1)
  from spartan_amd import expr
  from spartan_amd.examples.fuzzy_kmeans import fuzzy_kmeans
  r = np.random.RandomState(11)
  X = np.concatenate([r.randn(100, 5) + 4 * c for c in range(3)]).astype(dtype)
  C0 = X[[0, 150, 250]].astype(np.float64) + 0.1
  want_labels, want_C = fuzzy_kmeans_loop(X, C0, 2.0, 2)
  labels, centers = fuzzy_kmeans(expr.from_numpy(X, tile_hint=(128, 5)), k=3, num_iter=2, m=2.0, centers=C0,
                                 return_centers=True)
  assert np.array_equal(labels.glom(), want_labels)
  err = float(np.abs(centers - want_C).max() / np.abs(want_C).max())
  print('driver %s: centres relative error %.3g' % (np.dtype(dtype), err))
  assert err <= TOL[np.dtype(dtype)]
