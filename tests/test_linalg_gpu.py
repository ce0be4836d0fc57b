"""spx_potrf / spx_trsm / spx_syrk and the linalg expression layer on a real
MI355X, at the sizes where the blocking can go wrong: around
the diagonal block ``nb`` and the outer panel ``nb_outer`` (spx_potrf_plan).

Every numerical check is the derived bound of tests/linalg_ref.py (Higham,
Theorems 10.3 / 8.5), evaluated in np.longdouble; integer-valued data must come
out bit-exact.
"""
import numpy as np
import pytest

from linalg_ref import (assert_bound, exact_factor, potrf_ratio, same_bits, solve_ratio, spd_data, syrk_ratio)

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


def _sizes(dtype):
  from spartan_amd import backend
  nb, nbo = backend.potrf_plan(dtype)
  return [1, 2, nb - 1, nb, nb + 1, 2 * nb + 17, nbo - 1, nbo, nbo + 1, 2 * nbo + nb + 5]


def _dev(a):
  import torch
  return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _padded(a, pad, fill=np.nan):
  """(buffer, view): ``a`` as the leading columns of a ``fill``-ed buffer with
  ``pad`` more columns, on the device."""
  buf = np.full((a.shape[0], a.shape[1] + pad), fill, a.dtype)
  buf[:, :a.shape[1]] = a
  t = _dev(buf)
  return t, t[:, :a.shape[1]]


def _host(t):
  return t.cpu().numpy()


def _bits(a):
  return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


# ------------------------------------------------------------------ potrf
@pytest.mark.parametrize('si', range(10))
@pytest.mark.parametrize('kind', ['wishart', 'illcond', 'minij', 'diag'])
@pytest.mark.parametrize('dtype', DTYPES)
def test_potrf(gpu_ctx, dtype, kind, si):
  import torch
  from spartan_amd import backend
  be = backend.get()
  n = _sizes(dtype)[si]
  A = spd_data(kind, n, dtype, 3)
  dA = _dev(A)
  L = torch.full((n, n), 7.0, dtype=dA.dtype, device=dA.device)
  info = be.potrf(dA, L)
  Lh = _host(L)
  assert int(info.item()) == 0
  assert np.array_equal(_bits(_host(dA)), _bits(A))  # the input is untouched
  up = np.triu_indices(n, 1)
  assert not np.any(_bits(Lh)[up])  # the strict upper triangle is +0.0, bit for bit
  if kind in ('minij', 'diag'):
    assert same_bits(Lh, exact_factor(kind, n, dtype))
  else:
    assert_bound(potrf_ratio(A, Lh), 'potrf %s n=%d %s' % (kind, n, np.dtype(dtype)))
  # a repeat gives the same bits
  L2 = torch.empty_like(L)
  assert int(be.potrf(dA, L2).item()) == 0 and same_bits(_host(L2), Lh)
  # NaN above the diagonal of the input and in the pad of both matrices: the same bits
  dirty = A.copy()
  dirty[up] = np.nan
  abuf, aview = _padded(dirty, 3)
  lbuf, lview = _padded(np.zeros_like(A), 5)
  assert int(be.potrf(aview, lview).item()) == 0
  assert same_bits(_host(lview), Lh)
  assert np.all(np.isnan(_host(lbuf)[:, n:])) and np.all(np.isnan(_host(abuf)[:, n:]))
  # in place
  assert int(be.potrf(aview, aview).item()) == 0
  assert same_bits(_host(aview), Lh) and np.all(np.isnan(_host(abuf)[:, n:]))


@pytest.mark.parametrize('dtype', DTYPES)
def test_potrf_info(gpu_ctx, dtype):
  import torch
  from spartan_amd import backend
  be = backend.get()
  nb, nbo = backend.potrf_plan(dtype)
  for n, js in ((2 * nb + 17, (0, nb - 1, nb, 2 * nb + 16)), (nbo + nb + 5, (nbo - 1, nbo, nbo + nb + 4))):
    good = spd_data('wishart', n, dtype, 4)
    for j in js:
      for bad in (-1.0, np.nan):
        A = good.copy()
        A[j, j] = bad
        dA = _dev(A)
        assert int(be.potrf(dA, torch.empty_like(dA)).item()) == j + 1, (n, j, bad)
    dA = _dev(good)
    assert int(be.potrf(dA, torch.empty_like(dA)).item()) == 0  # a success afterwards


def test_backend_argument_checks(gpu_ctx):
  import torch
  from spartan_amd import backend
  be = backend.get()
  a = torch.eye(4, dtype=torch.float32, device='cuda')
  with pytest.raises(ValueError, match='square'):
    be.potrf(a[:3], a[:3])
  with pytest.raises(ValueError, match='dtype'):
    be.potrf(a, a.double())
  with pytest.raises(ValueError, match='float32 / float64'):
    be.potrf(a.long(), a.long())
  with pytest.raises(ValueError, match='stride'):
    be.potrf(a.t()[:, :], a.clone().t())
  with pytest.raises(ValueError, match='side'):
    be.trsm(a, a.clone(), side='X')
  with pytest.raises(ValueError, match='shape'):
    be.trsm(a, torch.ones((3, 2), device='cuda'))
  with pytest.raises(ValueError, match='shape'):
    be.syrk(a, a[:, :3].contiguous(), a.clone())
  with pytest.raises(ValueError, match='square'):
    be.syrk(a[:3], a, torch.ones((3, 4), device='cuda'), lower=True)


# ------------------------------------------------------------------- trsm
@pytest.mark.parametrize('trans', [False, True])
@pytest.mark.parametrize('side', ['L', 'R'])
@pytest.mark.parametrize('dtype', DTYPES)
def test_trsm(gpu_ctx, dtype, side, trans):
  from spartan_amd import backend
  be = backend.get()
  nb, _ = backend.potrf_plan(dtype)
  r = np.random.RandomState(5)
  for nl in (1, nb - 1, nb + 1, 2 * nb + 17):
    Lw = np.linalg.cholesky(spd_data('wishart', nl, np.float64, 6)).astype(dtype)
    Lw[np.triu_indices(nl, 1)] = np.nan  # L's strict upper triangle is never read
    for kind, Lm in (('wishart', Lw), ('minij', np.tril(np.ones((nl, nl), dtype)))):
      for nrhs in (1, 5, 130):
        shape = (nl, nrhs) if side == 'L' else (nrhs, nl)
        if kind == 'minij':
          Bm = r.randint(-4, 5, shape).astype(dtype)
        else:
          Bm = r.standard_normal(shape).astype(dtype)
        lbuf, lview = _padded(Lm, 2)
        bbuf, bview = _padded(Bm, 3)
        be.trsm(lview, bview, side=side, trans=trans)
        X = _host(bview)
        msg = 'trsm %s %s nl=%d nrhs=%d %s %s' % (side, 'T' if trans else 'N', nl, nrhs, kind, np.dtype(dtype))
        assert np.all(np.isnan(_host(bbuf)[:, shape[1]:])), msg  # the pad is untouched
        Lc = np.tril(np.nan_to_num(Lm))
        if kind == 'minij':  # integer data stays exact
          op = Lc.T if trans else Lc
          want = np.linalg.solve(op.astype(np.float64), Bm.astype(np.float64)) if side == 'L' else \
              np.linalg.solve(op.T.astype(np.float64), Bm.T.astype(np.float64)).T
          assert same_bits(X + dtype(0), np.round(want).astype(dtype) + dtype(0)), msg  # a zero's sign is free
        else:
          assert_bound(solve_ratio(Lc, X, Bm, side, trans), msg)
        # the contiguous form gives the same bits
        d = _dev(Bm)
        be.trsm(_dev(Lc), d, side=side, trans=trans)
        assert same_bits(_host(d), X), msg


# ------------------------------------------------------------------- syrk
@pytest.mark.parametrize('dtype', DTYPES)
def test_syrk_plain(gpu_ctx, dtype):
  from spartan_amd import backend
  be = backend.get()
  r = np.random.RandomState(8)
  for M, N, K in ((1, 1, 1), (37, 21, 5), (128, 128, 64), (129, 65, 33), (300, 150, 70), (130, 63, 513),
                  (64, 200, 2)):
    A = r.standard_normal((M, K)).astype(dtype)
    Bm = r.standard_normal((N, K)).astype(dtype)
    for C0 in (np.zeros((M, N), dtype), r.standard_normal((M, N)).astype(dtype)):
      abuf, av = _padded(A, 1)
      bbuf, bv = _padded(Bm, 2)
      cbuf, cv = _padded(C0, 3)
      be.syrk(av, bv, cv)
      assert_bound(syrk_ratio(C0, A, Bm, _host(cv)), 'syrk %s %s' % ((M, N, K), np.dtype(dtype)))
      assert np.all(np.isnan(_host(cbuf)[:, N:]))
      c2 = _dev(C0)
      be.syrk(_dev(A), _dev(Bm), c2)
      assert same_bits(_host(c2), _host(cv))


@pytest.mark.parametrize('dtype', DTYPES)
def test_syrk_lower_touches_nothing_above_the_diagonal(gpu_ctx, dtype):
  """The factorization's own use: the panel P = W[K:, :K] and the trailing
  block C = W[K:, K:] of one matrix W that is NaN everywhere else, the strict
  upper triangle of C included."""
  from spartan_amd import backend
  be = backend.get()
  r = np.random.RandomState(9)
  for M, K in ((1, 1), (127, 64), (128, 7), (129, 64), (300, 70)):
    n = M + K
    W = np.full((n, n), np.nan, dtype)
    P = r.standard_normal((M, K)).astype(dtype)
    C0 = np.tril(r.standard_normal((M, M))).astype(dtype)
    W[K:, :K] = P
    low = np.tril_indices(M)
    W[K:, K:][low] = C0[low]
    dW = _dev(W)
    be.syrk(dW[K:, :K], dW[K:, :K], dW[K:, K:], lower=True)
    got = _host(dW)
    touched = np.zeros((n, n), bool)
    touched[K:, K:][low] = True
    assert np.array_equal(_bits(got)[~touched], _bits(W)[~touched])  # NaNs and the panel: the same bits
    assert_bound(syrk_ratio(C0, P, P, got[K:, K:], lower=True), 'syrk lower M=%d K=%d %s' % (M, K, np.dtype(dtype)))


# ------------------------------------------------------- expression level
def _layouts(n):
  third = -(-n // 3)
  return [(n, n), (-(-n // 2),) * 2, (third, third), (64, 64), (40, n)]


@pytest.mark.parametrize('W', [1, 3])
@pytest.mark.parametrize('dtype', DTYPES)
def test_expr_cholesky_and_solves(gpu_workers, dtype, W):
  gpu_workers(W)
  from spartan_amd import backend, expr
  nb, _ = backend.potrf_plan(dtype)
  n = 2 * nb + 17
  A = spd_data('wishart', n, dtype, 11)
  Bm = np.random.RandomState(12).standard_normal((n, 5)).astype(dtype)
  for hint in _layouts(n) + ['replicated']:
    if hint == 'replicated':
      from spartan_amd.array import distarray
      a = expr.lazify(distarray.ReplicatedArray(_dev(A)))
    else:
      a = expr.from_numpy(A, tile_hint=hint)
    Le = expr.cholesky(a)
    L = Le.glom()
    assert L.dtype == np.dtype(dtype) and not np.any(_bits(L)[np.triu_indices(n, 1)])
    assert_bound(potrf_ratio(A, L), 'expr cholesky %s W=%d %s' % (hint, W, np.dtype(dtype)))
    for bh in (None, (n, 2), (40, 5)):
      for trans in (0, 1):
        X = expr.solve_triangular(Le, expr.from_numpy(Bm, tile_hint=bh), trans=trans).glom()
        assert_bound(solve_ratio(L, X, Bm, 'L', bool(trans)), 'expr solve %s %s' % (hint, bh))
    x = expr.cho_solve(Le, expr.from_numpy(Bm[:, 0].copy(), tile_hint=(40,))).glom()
    y = expr.solve_triangular(Le, expr.from_numpy(Bm[:, 0].copy()), trans=0).glom()
    assert_bound(solve_ratio(L, x.reshape(n, 1), y.reshape(n, 1), 'L', True), 'expr cho_solve %s' % (hint,))
  bad = A.copy()
  bad[nb, nb] = -1.0
  for hint in _layouts(n):
    with pytest.raises(np.linalg.LinAlgError, match='order %d is not' % (nb + 1)):
      expr.cholesky(expr.from_numpy(bad, tile_hint=hint)).force()


@pytest.mark.parametrize('dtype', DTYPES)
def test_expr_cholesky_three_by_three_outer_tiles(gpu_workers, dtype):
  gpu_workers(3)
  from spartan_amd import backend, expr
  _, nbo = backend.potrf_plan(dtype)
  t = nbo + 1
  n = 3 * t
  A = spd_data('wishart', n, dtype, 13)
  x = expr.from_numpy(A, tile_hint=(t, t)).force()
  assert len(x.tiles) == 9
  L = expr.cholesky(expr.lazify(x)).glom()
  assert not np.any(_bits(L)[np.triu_indices(n, 1)])
  assert_bound(potrf_ratio(A, L), 'expr cholesky 3 x 3 tiles of %d %s' % (t, np.dtype(dtype)))


def test_reference_benchmark_check(gpu_workers):
  """tests/test_cholesky.py of the reference: A = dot(randn, randn.T), then
  np.isclose(A, L L^T) everywhere."""
  gpu_workers(3)
  from spartan_amd import expr
  from spartan_amd.examples.cholesky import cholesky
  n = 200
  g = expr.randn(n, n).force()
  A = expr.dot(expr.lazify(g), expr.from_numpy(np.ascontiguousarray(expr.lazify(g).glom().T))).force()
  L = cholesky(expr.lazify(A)).glom()
  assert np.all(np.isclose(expr.lazify(A).glom(), L.dot(L.T)))
  assert not np.any(np.triu(L, 1))
