"""spx_syevj and the eigh expression layer on a real MI355X, at
the sizes where the kernel can go wrong: n = 1 (no pair), even and odd n (the
phantom index), around one wave (63, 64, 65: the workgroup size and the lanes
per column change) and at the limit ``nmax`` of spx_syevj_plan.

Every numerical check is a ratio of tests/eigh_ref.py, evaluated in
np.longdouble and held to 4 x the yardstick that the NumPy model of the method
and LAPACK set on the same data kinds and sizes, plus the unconditional
envelope on the orthogonality.
"""
import ctypes

import numpy as np
import pytest

from eigh_ref import (KINDS, SWEEP_MAX, assert_ratios, check_drivers, check_form, eigh_data, same_bits, yardstick)

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


def _ns(dtype):
  from spartan_amd import backend
  nmax, _ = backend.syevj_plan(dtype)
  return [1, 2, 3, 4, 5, 17, 63, 64, 65, nmax - 1, nmax]


def _dev(a):
  import torch
  return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _host(t):
  return t.cpu().numpy()


def _bits(a):
  return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _run(A, uplo='L'):
  """(w, V, info) on the host of one syevj call on the host array ``A``."""
  from spartan_amd import backend
  w, V, info = backend.get().syevj(_dev(A), uplo)
  return _host(w), _host(V), _host(info)


# ------------------------------------------------------------------ syevj
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_syevj(gpu_ctx, dtype, kind):
  from spartan_amd import backend
  be = backend.get()
  _, sweep_max = backend.syevj_plan(dtype)
  assert sweep_max == SWEEP_MAX
  for n in _ns(dtype):
    what = 'syevj %s n=%d %s' % (kind, n, np.dtype(dtype))
    A, lam = eigh_data(kind, n, dtype)
    dA = _dev(A)
    w, V, info = be.syevj(dA)
    wh, Vh, ih = _host(w), _host(V), _host(info)
    assert np.array_equal(_bits(_host(dA)), _bits(A)), what  # the input is untouched
    assert wh.shape == (n,) and Vh.shape == (n, n) and ih.shape == (1,) and ih.dtype == np.int32
    sweeps = int(ih[0])
    assert 0 <= sweeps <= sweep_max, what
    check_form(wh, Vh)
    assert_ratios(A, wh, Vh, lam, sweeps, yardstick(dtype, n), what)
    # a repeat gives the same bits
    w2, V2, i2 = be.syevj(dA)
    assert same_bits(_host(w2), wh) and same_bits(_host(V2), Vh) and int(_host(i2)[0]) == sweeps, what
    # the exact cases
    if kind == 'zero':
      assert sweeps == 0 and not np.any(_bits(wh)) and np.array_equal(Vh, np.eye(n, dtype=dtype)), what
    elif n == 1:
      assert sweeps == 0 and same_bits(wh, A[0]) and Vh[0, 0] == 1, what
    elif kind == 'diag':
      assert sweeps == 1 and np.array_equal(wh, np.sort(np.diag(A))), what
      assert np.array_equal(np.sort(Vh, axis=0)[-1], np.ones(n, dtype)) and np.count_nonzero(Vh) == n, what
    elif kind == 'exchange':
      assert np.array_equal(wh, lam.astype(dtype)), what  # exactly -1, (0,) +1


@pytest.mark.parametrize('dtype', DTYPES)
def test_triangles(gpu_ctx, dtype):
  """Only the named triangle is read: NaN in the other one changes no bit;
  'U' on A is 'L' on A^T."""
  for n in (5, 17, 65):
    A, _ = eigh_data('gauss', n, dtype)
    w, V, info = _run(A)
    for uplo, unread in (('L', np.triu_indices(n, 1)), ('U', np.tril_indices(n, -1))):
      B = A.copy()
      B[unread] = np.nan
      w2, V2, i2 = _run(B, uplo)
      assert same_bits(w2, w) and same_bits(V2, V) and i2[0] == info[0], (n, uplo)
    M = np.random.RandomState(n).standard_normal((n, n)).astype(dtype)  # not symmetric: the triangles differ
    wu, Vu, iu = _run(M, 'U')
    wl, Vl, il = _run(np.ascontiguousarray(M.T), 'L')
    assert same_bits(wu, wl) and same_bits(Vu, Vl) and iu[0] == il[0], n
    assert not same_bits(wu, _run(M, 'L')[0]), n


@pytest.mark.parametrize('dtype', DTYPES)
def test_strides(gpu_ctx, dtype):
  """A, W and V as the leading columns of NaN-filled wider buffers, with a
  batch stride above n * lda: the same bits, the pads untouched (straight
  through the ABI: the backend allocates dense outputs)."""
  import torch
  from spartan_amd import backend
  be = backend.get()
  B = 3
  for n in (5, 17):
    mats = np.stack([eigh_data(k, n, dtype)[0] for k in ('gauss', 'posdef', 'tridiag')])
    want = [_run(m) for m in mats]
    abuf = np.full((B, n + 2, n + 3), np.nan, dtype)
    abuf[:, :n, :n] = mats
    ta = _dev(abuf)
    view = ta[:, :n, :n]
    assert view.stride(0) > n * view.stride(1)
    # the padded input through the backend
    w, V, info = be.syevj(view)
    for b in range(B):
      assert same_bits(_host(w)[b], want[b][0]) and same_bits(_host(V)[b], want[b][1]), (n, b)
      assert _host(info)[b] == want[b][2][0]
    assert np.array_equal(_bits(_host(ta)), _bits(abuf))  # A and its pads untouched
    # padded outputs through the ABI
    tw = _dev(np.full((B, n + 4), np.nan, dtype))
    tv = _dev(np.full((B, n + 1, n + 5), np.nan, dtype))
    ti = torch.full((B,), 77, dtype=torch.int32, device='cuda')
    rc = be.lib.spx_syevj(backend.spx_dtype(dtype), 0, B, n, ctypes.c_void_p(view.data_ptr()), n + 3,
                          (n + 2) * (n + 3), ctypes.c_void_p(tw.data_ptr()), n + 4, ctypes.c_void_p(tv.data_ptr()),
                          n + 5, (n + 1) * (n + 5), ctypes.c_void_p(ti.data_ptr()), be.stream())
    assert rc == 0
    hw, hv = _host(tw), _host(tv)
    for b in range(B):
      assert same_bits(hw[b, :n], want[b][0]) and same_bits(hv[b, :n, :n], want[b][1]), (n, b)
      assert _host(ti)[b] == want[b][2][0]
    assert np.all(np.isnan(hw[:, n:])) and np.all(np.isnan(hv[:, n:, :])) and np.all(np.isnan(hv[:, :n, n:]))
    assert np.array_equal(_bits(_host(ta)), _bits(abuf))


@pytest.mark.parametrize('dtype', DTYPES)
def test_batch(gpu_ctx, dtype):
  """Every matrix of a batch gives the bits of its own batch-1 call, fast and
  slow matrices mixed; a NaN matrix gives -1 and NaN for itself only."""
  from spartan_amd import backend
  be = backend.get()
  for n in (5, 17):
    base = [eigh_data(k, n, dtype, s)[0] for k, s in (('diag', 0), ('zero', 0), ('posdef', 0), ('gauss', 0),
                                                      ('gauss', 1), ('exchange', 0), ('posdef', 1), ('tridiag', 0))]
    single = [_run(m) for m in base]
    assert len({int(s[2][0]) for s in single}) >= 3  # fast and slow matrices side by side
    for B in (3, 257):  # 257: one more than the CU count
      stack = np.stack([base[b % len(base)] for b in range(B)])
      w, V, info = (_host(t) for t in be.syevj(_dev(stack)))
      assert w.shape == (B, n) and V.shape == (B, n, n) and info.shape == (B,)
      for b in range(B):
        ws, Vs, is_ = single[b % len(base)]
        assert same_bits(w[b], ws) and same_bits(V[b], Vs) and info[b] == is_[0], (n, B, b)
      bad = stack.copy()
      bad[B // 2, n - 1, 0] = np.nan
      w2, V2, info2 = (_host(t) for t in be.syevj(_dev(bad)))
      for b in range(B):
        if b == B // 2:
          assert info2[b] == -1 and np.all(np.isnan(w2[b])) and np.all(np.isnan(V2[b])), (n, B)
        else:
          assert same_bits(w2[b], w[b]) and same_bits(V2[b], V[b]) and info2[b] == info[b], (n, B, b)
  # +-inf counts as not finite too; an empty batch and n == 0 launch nothing
  A = eigh_data('gauss', 4, dtype)[0]
  A[2, 1] = -np.inf
  w, V, info = _run(A)
  assert info[0] == -1 and np.all(np.isnan(w)) and np.all(np.isnan(V))
  w, V, info = be.syevj(_dev(np.zeros((0, 4, 4), dtype)))
  assert tuple(w.shape) == (0, 4) and tuple(V.shape) == (0, 4, 4) and tuple(info.shape) == (0,)
  w, V, info = be.syevj(_dev(np.zeros((0, 0), dtype)))
  assert tuple(w.shape) == (0,) and tuple(V.shape) == (0, 0)


def test_backend_argument_checks(gpu_ctx):
  import torch
  from spartan_amd import backend
  be = backend.get()
  a = torch.eye(4, dtype=torch.float32, device='cuda')
  with pytest.raises(ValueError, match='2-d or 3-d'):
    be.syevj(a[0])
  with pytest.raises(ValueError, match='2-d or 3-d'):
    be.syevj(a.reshape(1, 1, 4, 4))
  with pytest.raises(ValueError, match='square'):
    be.syevj(a[:3])
  with pytest.raises(ValueError, match='square'):
    be.syevj(torch.ones((2, 3, 4), device='cuda'))
  for dt, tdt in ((np.float32, torch.float32), (np.float64, torch.float64)):
    nmax, _ = backend.syevj_plan(dt)
    with pytest.raises(ValueError, match='limit %d' % nmax):
      be.syevj(torch.ones((nmax + 1, nmax + 1), dtype=tdt, device='cuda'))
  with pytest.raises(ValueError, match='float32 / float64'):
    be.syevj(a.long())
  with pytest.raises(ValueError, match='stride'):
    be.syevj(torch.ones((4, 8), device='cuda').t()[:4, :4])
  with pytest.raises(ValueError, match='stride'):
    be.syevj(torch.ones((4, 8), device='cuda')[:, ::2])
  with pytest.raises(ValueError, match='uplo'):
    be.syevj(a, 'X')
  w, V, info = be.syevj(a.unsqueeze(0).expand(3, 4, 4))  # a zero batch stride: the same matrix three times
  assert tuple(w.shape) == (3, 4) and _host(info).tolist() == [1, 1, 1]


# ------------------------------------------------------- expression level
@pytest.mark.parametrize('W', [1, 3])
@pytest.mark.parametrize('dtype', DTYPES)
def test_expr_eigh(gpu_workers, dtype, W):
  gpu_workers(W)
  from spartan_amd import backend, expr
  from spartan_amd.array import distarray
  nmax, _ = backend.syevj_plan(dtype)
  for n in (17, nmax):
    a, b = -(-2 * n // 5), -(-3 * n // 10)
    yard = yardstick(dtype, n)
    for kind in ('gauss', 'rankdef'):
      A, lam = eigh_data(kind, n, dtype)
      first = None
      for hint in [(n, n), (a, n), (n, b), (a, b), 'replicated']:
        x = distarray.ReplicatedArray(_dev(A)) if hint == 'replicated' else expr.from_numpy(A, tile_hint=hint).force()
        we, ve = expr.eigh(expr.lazify(x))
        assert we.shape == (n,) and ve.shape == (n, n)
        wa, va = we.force(), ve.force()
        assert isinstance(wa, distarray.ReplicatedArray) and isinstance(va, distarray.ReplicatedArray)
        w, V = wa.glom(), va.glom()
        check_form(w, V)
        if first is None:
          assert_ratios(A, w, V, lam, None, yard, 'expr eigh %s %s W=%d n=%d %s' % (kind, hint, W, n, np.dtype(dtype)))
          first = (w, V)
        assert same_bits(w, first[0]) and same_bits(V, first[1]), (n, kind, hint)  # the same bits for every layout
  # a stack
  n = 17
  kinds = ('gauss', 'diag', 'zero', 'posdef', 'exchange')
  S = np.stack([eigh_data(k, n, dtype)[0] for k in kinds])
  lams = [eigh_data(k, n, dtype)[1] for k in kinds]
  yard = yardstick(dtype, n)
  first = None
  for hint in [(5, n, n), (2, n, n), (3, 12, n), (2, n, 6), 'replicated']:
    x = distarray.ReplicatedArray(_dev(S)) if hint == 'replicated' else expr.from_numpy(S, tile_hint=hint).force()
    we, ve = expr.eigh(expr.lazify(x))
    assert we.shape == (5, n) and ve.shape == (5, n, n)
    va = ve.force()
    if hint != 'replicated':
      assert va.tiles == x.tiles
    w, V = we.glom(), va.glom()
    if first is None:
      for i in range(5):
        check_form(w[i], V[i])
        assert_ratios(S[i], w[i], V[i], lams[i], None, yard, 'expr eigh stack %s W=%d matrix %d' % (hint, W, i))
      first = (w, V)
    assert same_bits(w, first[0]) and same_bits(V, first[1]), hint
  bad = S.copy()
  bad[3, 5, 2] = np.nan
  for hint in [(2, n, n), (3, 12, n)]:
    with pytest.raises(np.linalg.LinAlgError, match='Eigenvalues did not converge'):
      expr.eigh(expr.from_numpy(bad, tile_hint=hint))[0].force()
  with pytest.raises(np.linalg.LinAlgError, match='Eigenvalues did not converge'):
    expr.eigvalsh(expr.from_numpy(bad[3], tile_hint=(6, n))).force()


@pytest.mark.parametrize('W', [1, 3])
def test_reference_svds_and_lanczos(gpu_workers, W):
  """The reference's test_svds restated on a dense float64 matrix, on the real
  backend."""
  gpu_workers(W)
  check_drivers(W)
