"""spx_gesvj and the svd expression layer on a real MI355X, at
the sizes where the kernel can go wrong: n = 1 (no pair), even and odd n (the
phantom index), around one wave (63, 64, 65: the workgroup size and the lanes
per pair change), at the column limit ``nmax`` and, for n = 17 and 64, at the
row limit ``mmax`` of spx_gesvj_plan (both ends of the LDS budget).

Every numerical check is a ratio of tests/svd_ref.py, evaluated in
np.longdouble and held to 4 x the yardstick that the NumPy model of the method
and LAPACK set on the same data kinds and sizes, plus the unconditional
envelope on the orthogonality of Vt.
"""
import ctypes

import numpy as np
import pytest

from svd_ref import (KINDS, SWEEP_MAX, TALL_KINDS, assert_ratios, assert_rel, check_form, dup_columns, low_rank,
                     same_bits, svd_data, svd_ratios, tall_yardstick, yardstick, FACTOR)

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


def _sizes(dtype):
  from spartan_amd import backend
  nmax = backend.gesvj_plan(dtype, 1)[0]
  sq = [1, 2, 3, 4, 5, 17, 63, 64, 65, nmax - 1, nmax]
  return [(n, n) for n in sq] + [(2, 1), (65, 17), (backend.gesvj_plan(dtype, 17)[1], 17),
                                 (backend.gesvj_plan(dtype, 64)[1], 64)]


def _dev(a):
  import torch
  return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _host(t):
  return t.cpu().numpy()


def _bits(a):
  return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _run(A):
  """(U, s, Vt, info) on the host of one gesvj call on the host array ``A``."""
  from spartan_amd import backend
  return tuple(_host(t) for t in backend.get().gesvj(_dev(A)))


def _same(a, b):
  return all(same_bits(x, y) for x, y in zip(a, b))


# ------------------------------------------------------------------ gesvj
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_gesvj(gpu_ctx, dtype, kind):
  from spartan_amd import backend
  be = backend.get()
  sweep_max = backend.gesvj_plan(dtype, 1)[2]
  assert sweep_max == SWEEP_MAX
  for m, n in _sizes(dtype):
    what = 'gesvj %s (%d, %d) %s' % (kind, m, n, np.dtype(dtype))
    A, sigma = svd_data(kind, m, n, dtype)
    dA = _dev(A)
    U, s, Vt, info = be.gesvj(dA)
    Uh, sh, Vh, ih = _host(U), _host(s), _host(Vt), _host(info)
    assert np.array_equal(_bits(_host(dA)), _bits(A)), what  # the input is untouched
    assert Uh.shape == (m, n) and sh.shape == (n,) and Vh.shape == (n, n) and ih.shape == (1,), what
    assert ih.dtype == np.int32
    sweeps = int(ih[0])
    assert 0 <= sweeps <= sweep_max, what
    check_form(sh, Vh)
    assert_ratios(A, Uh, sh, Vh, sigma, sweeps, yardstick(dtype, m, n), what)
    if kind == 'graded':
      assert_rel(sh, m, n, dtype, what)
    # a repeat gives the same bits; jobu = 0 gives the same bits of S
    again = tuple(_host(t) for t in be.gesvj(dA))
    assert _same(again, (Uh, sh, Vh, ih)), what
    U0, s0, Vt0, i0 = be.gesvj(dA, compute_uv=False)
    assert U0 is None and Vt0 is None and same_bits(_host(s0), sh) and int(_host(i0)[0]) == sweeps, what
    # the exact cases
    zeros = np.flatnonzero(sh == 0)
    assert not np.any(Uh[:, zeros]), what
    if kind == 'zero':
      assert sweeps == 0 and not np.any(_bits(sh)) and not np.any(_bits(Uh)), what
      assert np.array_equal(Vh, np.eye(n, dtype=dtype)), what
    elif n == 1:
      assert sweeps == 0 and Vh[0, 0] == 1, what
    elif kind == 'diag':
      assert sweeps == 1 and np.array_equal(sh, sigma.astype(dtype)), what  # one sweep, sorted |d| exactly
      assert np.count_nonzero(Vh) == n and np.array_equal(np.abs(Vh).sum(0), np.ones(n, dtype)), what
      assert np.array_equal(np.abs(Vh).sum(1), np.ones(n, dtype)), what  # Vt: a (signed) permutation
    elif kind == 'dup':
      assert zeros.size == (1 if dup_columns(n)[2] is None else 2), what  # the equal pair and the zero column
    elif kind == 'ones':
      assert zeros.size == n - 1, what


@pytest.mark.parametrize('dtype', DTYPES)
def test_strides(gpu_ctx, dtype):
  """A, U, S and Vt as the leading columns of NaN-filled wider buffers, with
  batch strides above the dense ones: the same bits, the pads untouched
  (straight through the ABI: the backend allocates dense outputs)."""
  import torch
  from spartan_amd import backend
  be = backend.get()
  B = 3
  for m, n in ((7, 5), (17, 17)):
    mats = np.stack([svd_data(k, m, n, dtype)[0] for k in ('gauss', 'illcond', 'dup')])
    want = [_run(x) for x in mats]
    abuf = np.full((B, m + 2, n + 3), np.nan, dtype)
    abuf[:, :m, :n] = mats
    ta = _dev(abuf)
    view = ta[:, :m, :n]
    assert view.stride(0) > m * view.stride(1)
    # the padded input through the backend
    got = tuple(_host(t) for t in be.gesvj(view))
    for b in range(B):
      assert _same([g[b] for g in got[:3]], want[b][:3]) and got[3][b] == want[b][3][0], (m, n, b)
    assert np.array_equal(_bits(_host(ta)), _bits(abuf))  # A and its pads untouched
    # padded outputs through the ABI
    tu = _dev(np.full((B, m + 1, n + 2), np.nan, dtype))
    ts = _dev(np.full((B, n + 4), np.nan, dtype))
    tv = _dev(np.full((B, n + 1, n + 5), np.nan, dtype))
    ti = torch.full((B,), 77, dtype=torch.int32, device='cuda')
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    for jobu in (1, 0):
      ts.fill_(float('nan'))
      rc = be.lib.spx_gesvj(backend.spx_dtype(dtype), jobu, B, m, n, ptr(view), n + 3, (m + 2) * (n + 3),
                            ptr(tu) if jobu else None, n + 2, (m + 1) * (n + 2), ptr(ts), n + 4,
                            ptr(tv) if jobu else None, n + 5, (n + 1) * (n + 5), ptr(ti), be.stream())
      assert rc == 0
      hu, hs, hv = _host(tu), _host(ts), _host(tv)
      for b in range(B):
        assert same_bits(hu[b, :m, :n], want[b][0]) and same_bits(hs[b, :n], want[b][1]), (m, n, b, jobu)
        assert same_bits(hv[b, :n, :n], want[b][2]) and _host(ti)[b] == want[b][3][0], (m, n, b, jobu)
      assert np.all(np.isnan(hs[:, n:])) and np.all(np.isnan(hu[:, m:, :])) and np.all(np.isnan(hu[:, :m, n:]))
      assert np.all(np.isnan(hv[:, n:, :])) and np.all(np.isnan(hv[:, :n, n:]))
      assert np.array_equal(_bits(_host(ta)), _bits(abuf))


@pytest.mark.parametrize('dtype', DTYPES)
def test_batch(gpu_ctx, dtype):
  """Every matrix of a batch gives the bits of its own batch-1 call, fast and
  slow matrices mixed; a NaN matrix gives -1 and NaN for itself only."""
  from spartan_amd import backend
  be = backend.get()
  for m, n in ((7, 5), (17, 17)):
    base = [svd_data(k, m, n, dtype, s)[0] for k, s in (('diag', 0), ('zero', 0), ('illcond', 0), ('gauss', 0),
                                                        ('gauss', 1), ('ones', 0), ('rankdef', 1), ('dup', 0))]
    single = [_run(x) for x in base]
    assert len({int(s[3][0]) for s in single}) >= 3  # fast and slow matrices side by side
    for B in (3, 257):  # 257: one more than the CU count
      stack = np.stack([base[b % len(base)] for b in range(B)])
      U, s, Vt, info = (_host(t) for t in be.gesvj(_dev(stack)))
      assert U.shape == (B, m, n) and s.shape == (B, n) and Vt.shape == (B, n, n) and info.shape == (B,)
      for b in range(B):
        assert _same((U[b], s[b], Vt[b]), single[b % len(base)][:3]), (m, n, B, b)
        assert info[b] == single[b % len(base)][3][0], (m, n, B, b)
      bad = stack.copy()
      bad[B // 2, m - 1, 0] = np.nan
      U2, s2, Vt2, info2 = (_host(t) for t in be.gesvj(_dev(bad)))
      for b in range(B):
        if b == B // 2:
          assert info2[b] == -1 and all(np.all(np.isnan(x[b])) for x in (U2, s2, Vt2)), (m, n, B)
        else:
          assert _same((U2[b], s2[b], Vt2[b]), (U[b], s[b], Vt[b])) and info2[b] == info[b], (m, n, B, b)
      s3, i3 = (_host(be.gesvj(_dev(bad), compute_uv=False)[i]) for i in (1, 3))
      assert same_bits(s3, s2) and np.array_equal(i3, info2), (m, n, B)
  # +-inf counts as not finite too; an empty batch and n == 0 launch nothing
  A = svd_data('gauss', 6, 4, dtype)[0]
  A[2, 1] = -np.inf
  U, s, Vt, info = _run(A)
  assert info[0] == -1 and np.all(np.isnan(U)) and np.all(np.isnan(s)) and np.all(np.isnan(Vt))
  U, s, Vt, info = be.gesvj(_dev(np.zeros((0, 6, 4), dtype)))
  assert tuple(U.shape) == (0, 6, 4) and tuple(s.shape) == (0, 4) and tuple(Vt.shape) == (0, 4, 4)
  assert tuple(info.shape) == (0,)
  U, s, Vt, info = be.gesvj(_dev(np.zeros((3, 0), dtype)))
  assert tuple(U.shape) == (3, 0) and tuple(s.shape) == (0,) and tuple(Vt.shape) == (0, 0)


def test_backend_argument_checks(gpu_ctx):
  import torch
  from spartan_amd import backend
  be = backend.get()
  a = torch.eye(4, dtype=torch.float32, device='cuda')
  with pytest.raises(ValueError, match='2-d or 3-d'):
    be.gesvj(a[0])
  with pytest.raises(ValueError, match='2-d or 3-d'):
    be.gesvj(a.reshape(1, 1, 4, 4))
  with pytest.raises(ValueError, match='m >= n'):
    be.gesvj(a[:3])
  with pytest.raises(ValueError, match='m >= n'):
    be.gesvj(torch.ones((2, 3, 4), device='cuda'))
  for dt, tdt in ((np.float32, torch.float32), (np.float64, torch.float64)):
    nmax, mmax, _ = backend.gesvj_plan(dt, 4)
    with pytest.raises(ValueError, match='limit %d' % nmax):
      be.gesvj(torch.ones((nmax + 1, nmax + 1), dtype=tdt, device='cuda'))
    with pytest.raises(ValueError, match='limit %d for n = 4' % mmax):
      be.gesvj(torch.ones((mmax + 1, 4), dtype=tdt, device='cuda'))
  with pytest.raises(ValueError, match='float32 / float64'):
    be.gesvj(a.long())
  with pytest.raises(ValueError, match='stride'):
    be.gesvj(torch.ones((4, 8), device='cuda').t()[:4, :4])
  with pytest.raises(ValueError, match='stride'):
    be.gesvj(torch.ones((4, 8), device='cuda')[:, ::2])
  U, s, Vt, info = be.gesvj(a.unsqueeze(0).expand(3, 4, 4))  # a zero batch stride: the same matrix three times
  assert tuple(s.shape) == (3, 4) and _host(info).tolist() == [1, 1, 1]
  assert np.array_equal(_host(s), np.ones((3, 4), np.float32))


# ------------------------------------------------------- expression level
def _triple(x):
  from spartan_amd import expr
  return tuple(e.force() for e in expr.svd(expr.lazify(x)))


@pytest.mark.parametrize('W', [1, 3])
@pytest.mark.parametrize('dtype', DTYPES)
def test_expr_svd_direct_and_stack(gpu_workers, dtype, W):
  gpu_workers(W)
  from spartan_amd import backend, expr
  from spartan_amd.array import distarray
  nmax = backend.gesvj_plan(dtype, 1)[0]
  for m, n in ((17, 17), (65, 17), (17, 65), (nmax, nmax)):
    a, b = -(-2 * m // 5), -(-3 * n // 10)
    tall = (max(m, n), min(m, n))
    yard = yardstick(dtype, *tall)
    for kind in ('gauss', 'rankdef'):
      T, sigma = svd_data(kind, tall[0], tall[1], dtype)
      A = T if m >= n else np.ascontiguousarray(T.T)
      first = None
      for hint in [(m, n), (a, n), (m, b), (a, b), 'replicated']:
        x = distarray.ReplicatedArray(_dev(A)) if hint == 'replicated' else expr.from_numpy(A, tile_hint=hint).force()
        arrs = _triple(x)
        assert all(isinstance(t, distarray.ReplicatedArray) for t in arrs)
        U, s, Vt = (t.glom() for t in arrs)
        k = min(m, n)
        assert U.shape == (m, k) and s.shape == (k,) and Vt.shape == (k, n)
        if first is None:
          what = 'expr svd %s %s W=%d (%d, %d) %s' % (kind, hint, W, m, n, np.dtype(dtype))
          if m >= n:
            check_form(s, Vt)
            assert_ratios(A, U, s, Vt, sigma, None, yard, what)
          else:  # the sign rule and the ratios on the transposed problem
            check_form(s, np.ascontiguousarray(U.T))
            assert_ratios(T, np.ascontiguousarray(Vt.T), s, np.ascontiguousarray(U.T), sigma, None, yard, what)
          first = (U, s, Vt)
        assert _same((U, s, Vt), first), (m, n, kind, hint)  # the same bits for every layout
      # svd(transpose(A)) is (Vt^T, s, U^T), bit for bit (m != n: the transpose of a square matrix is a
      # tall-or-square problem of its own, solved as it stands); svdvals are the same bits
      Ut, st, Vtt = (e.glom() for e in expr.svd(expr.transpose(expr.from_numpy(A, tile_hint=(a, b)))))
      if m != n:
        assert same_bits(Ut, np.ascontiguousarray(first[2].T)) and same_bits(st, first[1]), (m, n, kind)
        assert same_bits(Vtt, np.ascontiguousarray(first[0].T)), (m, n, kind)
      else:
        check_form(st, Vtt)
        assert_ratios(np.ascontiguousarray(A.T), Ut, st, Vtt, sigma, None, yard, 'expr svd transposed %s' % kind)
      assert same_bits(expr.svdvals(expr.from_numpy(A, tile_hint=(a, n))).glom(), first[1]), (m, n, kind)
  # stacks of five kinds
  kinds = ('gauss', 'diag', 'zero', 'illcond', 'dup')
  for m, n in ((17, 17), (20, 6)):
    S = np.stack([svd_data(k, m, n, dtype)[0] for k in kinds])
    sigmas = [svd_data(k, m, n, dtype)[1] for k in kinds]
    yard = yardstick(dtype, m, n)
    first = None
    for hint in [(5, m, n), (2, m, n), (3, -(-2 * m // 3), n), (2, m, -(-n // 3)), 'replicated']:
      x = distarray.ReplicatedArray(_dev(S)) if hint == 'replicated' else expr.from_numpy(S, tile_hint=hint).force()
      Ue, se, Vte = expr.svd(expr.lazify(x))
      assert Ue.shape == (5, m, n) and se.shape == (5, n) and Vte.shape == (5, n, n)
      U, s, Vt = Ue.glom(), se.glom(), Vte.glom()
      if first is None:
        for i in range(5):
          check_form(s[i], Vt[i])
          assert_ratios(S[i], U[i], s[i], Vt[i], sigmas[i], None, yard,
                        'expr svd stack %s W=%d (%d, %d) matrix %d' % (hint, W, m, n, i))
        first = (U, s, Vt)
      assert _same((U, s, Vt), first), (m, n, hint)
    bad = S.copy()
    bad[3, 5, 2] = np.nan
    for hint in [(2, m, n), (3, -(-2 * m // 3), n)]:
      with pytest.raises(np.linalg.LinAlgError, match='SVD did not converge'):
        expr.svd(expr.from_numpy(bad, tile_hint=hint))[1].force()
    with pytest.raises(np.linalg.LinAlgError, match='SVD did not converge'):
      expr.svdvals(expr.from_numpy(bad[3], tile_hint=(6, n))).force()


@pytest.mark.parametrize('W', [1, 3])
@pytest.mark.parametrize('dtype', DTYPES)
def test_expr_svd_tall_and_wide(gpu_workers, dtype, W):
  """The tall route (TSQR, the SVD of R, U = Q U_R) and its wide mirror, held
  to svd_ref.tall_yardstick: LAPACK's ratios on the data itself plus qr_ref's
  measured yardstick for Q on ``res`` and ``orthU`` (the SUM of the two: U
  inherits Q's errors); no bit equality across layouts, the TSQR tree differs."""
  gpu_workers(W)
  from spartan_amd import backend, expr
  from spartan_amd.array import distarray
  nq = min(backend.geqr_plan(dtype, 1)[0], backend.gesvj_plan(dtype, 1)[0])  # the most columns the route takes
  r = backend.geqr_plan(dtype, nq)[1]
  mmax17 = backend.gesvj_plan(dtype, 17)[1]
  # (1000 rows of 17 columns fit one workgroup in both dtypes: the second size is 2 mmax instead)
  for m, n in ((mmax17 + 1, 17), (2 * mmax17, 17), (3 * r + 5, nq)):
    assert m > backend.gesvj_plan(dtype, n)[1]  # not the direct route
    yard = tall_yardstick(dtype, m, n)
    a, b = -(-m // 3), -(-2 * n // 3)
    short = (m - (n - 1)) // 2 + 1  # two slabs and a last one of n - 1 rows or fewer
    for kind in TALL_KINDS:
      A, sigma = svd_data(kind, m, n, dtype)
      for hint in [(a, n), (a, b), (short, n), 'replicated']:
        x = distarray.ReplicatedArray(_dev(A)) if hint == 'replicated' else expr.from_numpy(A, tile_hint=hint).force()
        if hint == (short, n):
          assert 0 < min(e.shape[0] for e in x.tiles) < n
        Ua, sa, Vta = _triple(x)
        assert isinstance(sa, distarray.ReplicatedArray) and isinstance(Vta, distarray.ReplicatedArray)
        if hint in [(a, n), (short, n)]:
          assert Ua.tiles == x.tiles  # U is tiled like A
        U, s, Vt = Ua.glom(), sa.glom(), Vta.glom()
        what = 'expr svd tall %s %s W=%d (%d, %d) %s' % (kind, hint, W, m, n, np.dtype(dtype))
        check_form(s, Vt)
        assert_ratios(A, U, s, Vt, sigma, None, yard, what)
        if hint != (a, n):
          continue
        # the wide mirror: the factors swapped, the same ratios
        U2, s2, Vt2 = (e.glom() for e in expr.svd(expr.transpose(expr.lazify(x))))
        assert U2.shape == (n, n) and s2.shape == (n,) and Vt2.shape == (n, m)
        check_form(s2, np.ascontiguousarray(U2.T))
        assert_ratios(A, np.ascontiguousarray(Vt2.T), s2, np.ascontiguousarray(U2.T), sigma, None, yard,
                      what + ' transposed')
    bad = svd_data('gauss', m, n, dtype)[0]
    bad[m - 1, n - 1] = np.nan
    with pytest.raises(np.linalg.LinAlgError, match='SVD did not converge'):
      expr.svd(expr.from_numpy(bad, tile_hint=(a, n)))[0].force()


@pytest.mark.parametrize('W', [1, 3])
@pytest.mark.parametrize('dtype', DTYPES)
def test_expr_pinv(gpu_workers, dtype, W):
  """``pinv`` against NumPy's in double: for perturbations that keep the rank,
  |pinv(A + E) - pinv(A)| <= about 3 |pinv(A)|^2 |E| (Wedin), with |E| the
  backward error FACTOR x yardstick x u x |A| of the triple."""
  gpu_workers(W)
  from spartan_amd import expr
  eps = float(np.finfo(dtype).eps)
  for (m, n), kind in (((65, 17), 'gauss'), ((65, 17), 'rankdef'), ((17, 17), 'gauss'), ((9, 4), 'zero')):
    A, _ = svd_data(kind, m, n, dtype)
    yard = yardstick(dtype, m, n)
    for M, hint in ((A, (-(-m // 3), n)), (np.ascontiguousarray(A.T), (n, -(-m // 3)))):
      P = expr.pinv(expr.from_numpy(M, tile_hint=hint))
      assert P.shape == M.shape[::-1] and P.dtype == np.dtype(dtype)
      got = P.glom()
      if kind == 'zero':
        assert not np.any(got)
        continue
      want = np.linalg.pinv(M.astype(np.float64), rcond=max(m, n) * eps)
      s = np.linalg.svd(M.astype(np.float64), compute_uv=False)
      live = s[s > max(m, n) * eps * s[0]]
      bound = 3 * FACTOR * max(yard[:3]) * (eps / 2) * s[0] / live[-1] ** 2
      err = np.abs(got - want).max()
      print('pinv %s (%d, %d) %s W=%d: error %.3g, bound %.3g' % (kind, M.shape[0], M.shape[1], np.dtype(dtype), W,
                                                                 err, bound))
      assert err <= bound, (kind, M.shape)


@pytest.mark.parametrize('W', [1, 3])
def test_low_rank_singular_values(gpu_workers, W):
  """The driver-level check: on eigh_ref's low-rank matrices (the data of the
  reference's test_svds) ``svd`` recovers the prescribed singular values 6..3,
  and the rest are at most FACTOR x yardstick x u x 6."""
  gpu_workers(W)
  from spartan_amd import expr
  u = 2.0 ** -53
  for (m, n), k in (((80, 30), 6), ((60, 24), 10)):
    dense = low_rank(m, n, k, k)
    yard = yardstick(np.float64, m, n)
    s = expr.svdvals(expr.from_numpy(dense, tile_hint=(-(-m // W), n))).glom()
    assert s.shape == (n,)
    tol = FACTOR * yard[3] * u * 6
    print('low rank (%d, %d): largest deviation %.3g, tail %.3g, allowed %.3g'
          % (m, n, np.abs(s[:k + 1] - np.linspace(6, 3, k + 1)).max(), s[k + 1:].max(), tol))
    # (the matrix was formed in double from orthonormal factors of NumPy's qr: it carries their u-level errors,
    # which the yardstick's own sv ratio, measured on data with a prescribed spectrum, allows for)
    assert np.abs(s[:k + 1] - np.linspace(6, 3, k + 1)).max() <= tol
    assert s[k + 1:].max() <= tol
