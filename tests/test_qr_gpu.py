"""spx_geqr / spx_orgqr and the qr expression layer on a real MI355X (DESIGN.md
3.19), at the sizes where the tree can go wrong: around the block height
``r`` and the column limit ``nmax`` of spx_geqr_plan, one, two and three
levels.

Every numerical check is a ratio of tests/qr_ref.py, evaluated in
np.longdouble and held to 4 x the yardstick that LAPACK's Householder QR sets
on the same data kinds and sizes.
"""
import numpy as np
import pytest

from qr_ref import KINDS, assert_ratios, check_r, qr_data, qr_ratios, same_bits, yardstick

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


def _ns(dtype):
  from spartan_amd import backend
  nmax, _ = backend.geqr_plan(dtype, 1)
  return [1, 3, 17, nmax - 1, nmax]


def _ms(dtype, n):
  from spartan_amd import backend
  nmax, r = backend.geqr_plan(dtype, n)
  ms = [n, n + 1, r - 1, r, r + 1, 2 * r + 17]
  if n == nmax:
    ms.append((r // n + 1) * r + 1)  # the smallest m that needs three levels
  return sorted(set(m for m in ms if m >= n))


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


# ------------------------------------------------------------ geqr / orgqr
@pytest.mark.parametrize('kind', KINDS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_geqr_orgqr(gpu_ctx, dtype, kind):
  import torch
  from spartan_amd import backend
  be = backend.get()
  rs = np.random.RandomState(4)
  for n in _ns(dtype):
    ms = _ms(dtype, n)
    yard = yardstick(dtype, n, ms)
    for m in ms:
      what = 'geqr %s %dx%d %s' % (kind, m, n, np.dtype(dtype))
      A = qr_data(kind, m, n, dtype)
      dA = _dev(A)
      R, h = be.geqr(dA)
      Q = torch.full((m, n), 7.0, dtype=dA.dtype, device=dA.device)
      be.orgqr(h, None, Q)
      Rh, Qh = _host(R), _host(Q)
      assert np.array_equal(_bits(_host(dA)), _bits(A)), what  # the input is untouched
      check_r(Rh, bits=True)
      assert_ratios(A, Qh, Rh, yard, what)
      # a repeat gives the same bits
      R2, h2 = be.geqr(dA)
      Q2 = torch.empty_like(Q)
      be.orgqr(h2, None, Q2)
      assert same_bits(_host(R2), Rh) and same_bits(_host(Q2), Qh), what
      # with an explicit seed: orgqr(None) @ C, to the residual yardstick columnwise
      C = rs.standard_normal((n, n)).astype(dtype)
      QC = torch.empty_like(Q)
      be.orgqr(h, _dev(C), QC)
      want = Qh.astype(np.longdouble).dot(C.astype(np.longdouble))
      diff = np.sqrt(((_host(QC).astype(np.longdouble) - want) ** 2).sum(0))
      cn = np.sqrt((C.astype(np.longdouble) ** 2).sum(0))
      u = 2.0 ** -24 if dtype == np.float32 else 2.0 ** -53
      seeded = float(np.max(diff / (u * cn)))
      print('%s seeded: %.3g u (yardstick %.3g)' % (what, seeded, yard[0]))
      assert seeded <= 4 * yard[0], what
      # A, R, C and Q as the leading columns of NaN-filled buffers: the same bits, the pads untouched
      abuf, av = _padded(A, 3)
      qbuf, qv = _padded(np.zeros_like(A), 5)
      Rp, hp = be.geqr(av)
      be.orgqr(hp, None, qv)
      assert same_bits(_host(Rp), Rh) and same_bits(_host(qv), Qh), what
      assert np.all(np.isnan(_host(abuf)[:, n:])) and np.all(np.isnan(_host(qbuf)[:, n:])), what
      cbuf, cv = _padded(C, 2)
      qbuf2, qv2 = _padded(np.zeros_like(A), 1)
      be.orgqr(hp, cv, qv2)
      assert same_bits(_host(qv2), _host(QC)), what
      assert np.all(np.isnan(_host(qbuf2)[:, n:])) and np.all(np.isnan(_host(cbuf)[:, n:])), what


@pytest.mark.parametrize('dtype', DTYPES)
def test_padded_r_through_the_abi(gpu_ctx, dtype):
  """R with a leading dimension above n (the backend always allocates a dense
  R): straight through spx_geqr."""
  import ctypes
  import torch
  from spartan_amd import backend
  be = backend.get()
  nmax, r = backend.geqr_plan(dtype, 17)
  m, n = 2 * r + 17, 17
  A = qr_data('gauss', m, n, dtype)
  dA = _dev(A)
  want, _ = be.geqr(dA)
  rbuf, rv = _padded(np.zeros((n, n), dtype), 4)
  need = be.lib.spx_geqr_workspace(backend.spx_dtype(dtype), m, n)
  ws = torch.empty((need,), dtype=torch.uint8, device='cuda')
  rc = be.lib.spx_geqr(backend.spx_dtype(dtype), m, n, ctypes.c_void_p(dA.data_ptr()), n,
                       ctypes.c_void_p(rv.data_ptr()), n + 4, ctypes.c_void_p(ws.data_ptr()), need, be.stream())
  assert rc == 0
  assert same_bits(_host(rv), _host(want)) and np.all(np.isnan(_host(rbuf)[:, n:]))


@pytest.mark.parametrize('dtype', DTYPES)
def test_all_zero_matrix(gpu_ctx, dtype):
  import torch
  from spartan_amd import backend
  be = backend.get()
  for n in (3, 17):
    nmax, r = backend.geqr_plan(dtype, n)
    m = r + 1
    A = np.zeros((m, n), dtype)
    R, h = be.geqr(_dev(A))
    Q = torch.empty((m, n), dtype=R.dtype, device='cuda')
    be.orgqr(h, None, Q)
    assert not np.any(_bits(_host(R)))  # exactly zero
    Qh = _host(Q)
    assert np.all(np.isfinite(Qh))
    res, orth = qr_ratios(A, Qh, _host(R))
    yard = yardstick(dtype, n, _ms(dtype, n))
    print('zero %dx%d %s: orth %.3g u (yardstick %.3g)' % (m, n, np.dtype(dtype), orth, yard[1]))
    assert res == 0 and orth <= 4 * yard[1]


def test_backend_argument_checks(gpu_ctx):
  import torch
  from spartan_amd import backend
  be = backend.get()
  a = torch.ones((8, 4), dtype=torch.float32, device='cuda')
  with pytest.raises(ValueError, match='2-d'):
    be.geqr(a[0])
  with pytest.raises(ValueError, match='tall or square'):
    be.geqr(a[:3])
  nmax, _ = backend.geqr_plan(np.float32, 1)
  with pytest.raises(ValueError, match='limit %d' % nmax):
    be.geqr(torch.ones((nmax + 2, nmax + 1), dtype=torch.float32, device='cuda'))
  with pytest.raises(ValueError, match='float32 / float64'):
    be.geqr(a.long())
  with pytest.raises(ValueError, match='stride'):
    be.geqr(torch.ones((4, 8), device='cuda').t())
  R, h = be.geqr(a)
  with pytest.raises(ValueError, match='dtype'):
    be.orgqr(h, None, a.double())
  with pytest.raises(ValueError, match='dtype'):
    be.orgqr(h, R.double(), torch.empty_like(a))
  with pytest.raises(ValueError, match='shape'):
    be.orgqr(h, None, torch.empty((7, 4), device='cuda'))
  with pytest.raises(ValueError, match='shape'):
    be.orgqr(h, torch.ones((3, 3), device='cuda'), torch.empty_like(a))
  with pytest.raises(ValueError, match='stride'):
    be.orgqr(h, None, torch.empty((4, 8), device='cuda').t())
  with pytest.raises(ValueError, match='handle'):
    be.orgqr(None, None, torch.empty_like(a))


# ------------------------------------------------------- expression level
@pytest.mark.parametrize('W', [1, 3])
@pytest.mark.parametrize('dtype', DTYPES)
def test_expr_qr(gpu_workers, dtype, W):
  gpu_workers(W)
  from spartan_amd import backend, expr
  from spartan_amd.array import distarray
  nmax, _ = backend.geqr_plan(dtype, 1)
  for n in (17, nmax):
    _, r = backend.geqr_plan(dtype, n)
    m = 2 * r + 17
    yard = yardstick(dtype, n, (m,))
    for kind in ('gauss', 'rankdef'):
      A = qr_data(kind, m, n, dtype)
      for hint in [(m, n), (-(-m // 3), n), (40, n), (r + 1, -(-n // 2)), (64, 8), 'replicated']:
        if hint == 'replicated':
          x = distarray.ReplicatedArray(_dev(A))
        else:
          x = expr.from_numpy(A, tile_hint=hint).force()
        qe, re_ = expr.qr(expr.lazify(x))
        assert qe.shape == (m, n) and re_.shape == (n, n)
        q = qe.force()
        if hint != 'replicated':
          assert q.tiles == x.tiles  # A's tiling
        Q, R = q.glom(), re_.glom()
        assert Q.shape == A.shape and Q.dtype == A.dtype and R.dtype == A.dtype
        check_r(R)
        assert_ratios(A, Q, R, yard, 'expr qr %s %s W=%d %dx%d %s' % (kind, hint, W, m, n, np.dtype(dtype)))


# ------------------------------------------------- the reference's three tests
def test_reference_qr(gpu_workers):
  """tests/test_qr.py of the reference."""
  gpu_workers(3)
  from scipy import linalg
  from spartan_amd import expr
  from spartan_amd.examples.ssvd import qr
  Y = expr.randn(100, 10, tile_hint=(25, 10), dtype=np.float64).force()
  Q1, R1 = qr(Y)
  Q2, R2 = linalg.qr(Y.glom(), mode='economic')
  assert np.allclose(np.absolute(Q1.glom()), np.absolute(Q2))
  assert np.allclose(np.absolute(R1), np.absolute(R2))


def test_reference_ssvd(gpu_workers):
  """tests/test_ssvd.py of the reference."""
  gpu_workers(3)
  from spartan_amd import expr
  from spartan_amd.examples.ssvd import svd
  A = expr.randn(120, 30, tile_hint=(40, 30), dtype=np.float64)
  U, S, VT = svd(A)
  U2, S2, VT2 = np.linalg.svd(A.glom(), full_matrices=0)
  assert np.allclose(np.absolute(U.glom()), np.absolute(U2))
  assert np.allclose(np.absolute(S), np.absolute(S2))
  assert np.allclose(np.absolute(VT), np.absolute(VT2))


def test_reference_pca(gpu_workers):
  """tests/test_pca.py of the reference, against the top right singular
  vectors of the centred data (what sklearn's PCA computes)."""
  gpu_workers(3)
  from spartan_amd import expr
  from spartan_amd.examples.pca import PCA
  data = np.random.RandomState(0).randn(40, 20)
  A = expr.from_numpy(data, tile_hint=(14, 20))
  m = PCA(10)
  m.fit(A)
  want = np.linalg.svd(data - data.mean(0), full_matrices=False)[2][:10]
  assert np.allclose(np.absolute(m.components_), np.absolute(want))
