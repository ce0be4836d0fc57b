"""spx_csrmm / spx_csr_todense and the sparse expression layer on a real MI355X
(DESIGN.md 3.20), at the sizes where the kernel can go wrong: around the rows a
workgroup covers, the lanes of a row's group and the long-row threshold of
spx_csrmm_plan.

Integer-valued data (sparse_ref.exact_case) must equal scipy bit for bit;
random data must lie within the entrywise Higham bound of sparse_ref.bound,
which holds for every summation order.
"""
import numpy as np
import pytest

from sparse_ref import (KINDS, assert_within, dense_data, exact_case, reference, same_bits, sparse_data)

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
PS = [1, 2, 3, 4, 5, 17, 64, 65]
AB = [(1.0, 0.0), (2.5, 0.0), (1.0, 1.0), (-0.5, 0.75)]
PAD = 3


def _dev(a):
  import torch
  return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _host(t):
  return np.ascontiguousarray(t.cpu().numpy())


def _csr_dev(A):
  return _dev(A.indptr.astype(np.int64)), _dev(A.indices.astype(np.int32)), _dev(A.data)


def _padded(a, fill=np.nan):
  """(buffer, view): ``a`` as the leading columns of a NaN-filled wider device buffer."""
  buf = np.full((a.shape[0], a.shape[1] + PAD), fill, a.dtype)
  buf[:, :a.shape[1]] = a
  t = _dev(buf)
  return t, t[:, :a.shape[1]]


def _run(be, A, B, C0, alpha, beta, g=0, csr=None):
  """C of one csrmm call on fresh device copies; beta == 0: C starts as NaN."""
  csr = csr or _csr_dev(A)
  start = C0 if beta != 0 else np.full_like(C0, np.nan)
  C = _dev(start)
  be.csrmm(csr[0], csr[1], csr[2], A.shape[1], _dev(B), C, alpha, beta, g)
  return _host(C)


def _check_case(be, kind, m, n, p, dtype, what, g=0, **kw):
  """Every property of the issue's list for one matrix."""
  import torch
  from spartan_amd import backend
  for alpha, beta in AB:
    A, B, C0 = exact_case(kind, m, n, p, dtype, **kw)
    got = _run(be, A, B, C0, alpha, beta, g)
    assert same_bits(got, reference(A, B, C0, alpha, beta)), '%s exact alpha %g beta %g' % (what, alpha, beta)
  A = sparse_data(kind, m, n, dtype, **kw)
  B = dense_data(n, p, dtype)
  C0 = dense_data(m, p, dtype, seed=5)
  csr = _csr_dev(A)
  keep = [t.clone() for t in csr]
  for alpha, beta in AB:
    w = '%s alpha %g beta %g' % (what, alpha, beta)
    got = _run(be, A, B, C0, alpha, beta, g, csr)
    assert not np.isnan(got).any(), w  # beta == 0: C was NaN and is overwritten unread
    assert_within(got, A, B, C0, alpha, beta, w)
    assert same_bits(_run(be, A, B, C0, alpha, beta, g, csr), got), w + ': a second call'
    # a cached analysis (second and third call through one workspace) changes nothing
    ws = backend.CsrWorkspace()
    for _ in range(3):
      C = _dev(C0 if beta != 0 else np.full_like(C0, np.nan))
      be.csrmm(csr[0], csr[1], csr[2], n, _dev(B), C, alpha, beta, g, ws)
      assert same_bits(_host(C), got), w + ': cached workspace'
    # B and C as the leading columns of NaN-filled wider buffers
    bbuf, bview = _padded(B)
    cbuf, cview = _padded(C0 if beta != 0 else np.full_like(C0, np.nan))
    bkeep = bbuf.clone()
    be.csrmm(csr[0], csr[1], csr[2], n, bview, cview, alpha, beta, g)
    assert same_bits(_host(cview), got), w + ': padded'
    assert np.isnan(_host(cbuf[:, p:])).all() and torch.equal(bbuf[:, :p], bkeep[:, :p]), w
    assert np.isnan(_host(bbuf[:, p:])).all(), w
  for t, k in zip(csr, keep):
    assert torch.equal(t, k), what + ': the CSR arrays were written'


# --------------------------------------------------------------- be.csrmm
@pytest.mark.parametrize('p', PS)
@pytest.mark.parametrize('dtype', DTYPES)
def test_csrmm_rows_per_block(gpu_ctx, dtype, p):
  """Uniform rows of 8: m around the rows one workgroup covers."""
  from spartan_amd import backend
  be = backend.get()
  L, n = 8, 40
  g, _T, rpb = backend.csrmm_plan(dtype, 100, 100 * L, p)
  for m in sorted({1, 2, rpb - 1, rpb, rpb + 1, 3 * rpb + 5} - {0}):
    assert backend.csrmm_plan(dtype, m, m * L, p) == (g, _T, rpb)
    _check_case(be, 'uniform', m, n, p, dtype, 'uniform m=%d p=%d %s' % (m, p, np.dtype(dtype)), L=L)


def _lengths(T):
  gs = [1, 2, 4, 8, 16, 32, 64]
  return sorted({0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5} | {v for g in gs for v in (g - 1, g, g + 1)})


@pytest.mark.parametrize('g', [0, 1, 8, 64])
@pytest.mark.parametrize('p', [1, 3, 17, 65])
@pytest.mark.parametrize('dtype', DTYPES)
def test_csrmm_row_lengths(gpu_ctx, dtype, p, g):
  """Ragged rows of every length around g, the wave and the long-row threshold
  T, mixed in one matrix, with the plan's g and with forced ones."""
  from spartan_amd import backend
  be = backend.get()
  _, T, _ = backend.csrmm_plan(dtype, 1, 1, p)
  lens = _lengths(T)
  m, n = 2 * len(lens) + 1, 3 * T + 16
  _check_case(be, 'ragged', m, n, p, dtype, 'ragged p=%d g=%d %s' % (p, g, np.dtype(dtype)), g=g, lengths=lens)


@pytest.mark.parametrize('p', [1, 5, 64])
@pytest.mark.parametrize('dtype', DTYPES)
def test_csrmm_skew(gpu_ctx, dtype, p):
  """One row holds half of all nonzeros (several chunks of T) among short and
  empty rows."""
  from spartan_amd import backend
  be = backend.get()
  _, T, _ = backend.csrmm_plan(dtype, 1, 1, p)
  m = 2 * T + 4
  n = 3 * T + 16
  A = sparse_data('skew', m, n, dtype)
  assert np.diff(A.indptr).max() > T and np.diff(A.indptr).max() * 2 == A.nnz
  _check_case(be, 'skew', m, n, p, dtype, 'skew p=%d %s' % (p, np.dtype(dtype)))


@pytest.mark.parametrize('dtype', DTYPES)
def test_csrmm_other_kinds_and_empty(gpu_ctx, dtype):
  """diag, banded, onecol; nnz = 0 and matrices of empty rows give beta * C."""
  from spartan_amd import backend
  be = backend.get()
  for kind, m, n in (('diag', 70, 33), ('diag', 33, 70), ('banded', 300, 300), ('onecol', 67, 1)):
    for p in (1, 5):
      _check_case(be, kind, m, n, p, dtype, '%s %dx%d p=%d %s' % (kind, m, n, p, np.dtype(dtype)))
  for m in (1, 300):
    for p in (1, 5):
      A, B, C0 = exact_case('empty', m, 9, p, dtype)
      C0 = dense_data(m, p, dtype, seed=2)
      assert A.nnz == 0
      for alpha, beta in AB:
        got = _run(be, A, B, C0, alpha, beta)
        want = (np.dtype(dtype).type(beta) * C0) if beta != 0 else np.zeros_like(C0)
        assert np.array_equal(got, want), (m, p, alpha, beta)


# ------------------------------------------------------------- csr_todense
@pytest.mark.parametrize('dtype', DTYPES)
def test_csr_todense(gpu_ctx, dtype):
  import torch
  from spartan_amd import backend
  be = backend.get()
  _, T, _ = backend.csrmm_plan(dtype, 1, 1, 1)
  cases = [('empty', 5, 7, {}), ('diag', 70, 33, {}), ('diag', 33, 70, {}), ('uniform', 100, 40, {}),
           ('banded', 300, 300, {}), ('skew', 2 * T + 4, 3 * T + 16, {}), ('onecol', 67, 1, {}),
           ('ragged', 41, T + 40, {'lengths': [0, 1, 15, 16, 17, 64, T + 1]})]
  assert {c[0] for c in cases} == set(KINDS)
  for kind, m, n, kw in cases:
    A = sparse_data(kind, m, n, dtype, **kw)
    buf = torch.full((m, n + PAD), float('nan'), dtype=backend.torch_dtype(dtype), device='cuda')
    be.csr_todense(*_csr_dev(A), n, buf[:, :n])
    assert same_bits(_host(buf[:, :n]), A.toarray()), kind
    assert np.isnan(_host(buf[:, n:])).all(), kind


# -------------------------------------------------------- expression layer
def _spd(n, dtype=np.float64):
  import scipy.sparse as sp
  B = sp.random(n, n, density=0.03, format='csr', dtype=dtype, random_state=np.random.RandomState(2))
  Bs = (B + B.T).tocsr()
  s = 2 * abs(Bs).sum(1).max()
  return (s * sp.eye(n, dtype=dtype) + Bs).tocsr()


@pytest.mark.parametrize('W', [1, 3])
def test_expr_layer(gpu_workers, W):
  gpu_workers(W)
  from spartan_amd import expr
  from spartan_amd.examples.conj_gradient import cgit
  from spartan_amd.examples.pagerank import pagerank, site_graph
  from sparse_ref import LD, unit_roundoff
  for dtype in DTYPES:
    A = sparse_data('ragged', 203, 150, dtype, L=40)
    S = expr.from_numpy(A, tile_hint=(37, 150))
    assert len(S.force().tiles) == 6
    assert (S.glom() != A).nnz == 0
    for shape in ((150,), (150, 1), (150, 7)):
      X = dense_data(150, shape[1] if len(shape) == 2 else 1, dtype).reshape(shape)
      for operand in (X, expr.from_numpy(X), expr.from_numpy(X).force()):
        y = expr.dot(S, operand)
        got = y.glom()
        assert got.shape == A.dot(X).shape and got.dtype == dtype
        X2 = X.reshape(150, -1)
        assert_within(got.reshape(203, -1), A, X2, np.zeros((203, X2.shape[1]), dtype), 1.0, 0.0, 'dot %s' % (shape,))
    assert same_bits(expr.todense(S).glom(), A.toarray())
    ones = np.ones((150, 1), dtype)
    assert_within(expr.sum(S, axis=1).glom().reshape(203, 1), A, ones, np.zeros((203, 1), dtype), 1.0, 0.0, 'sum 1')
    # sum(None): the row sums within their bound, then a sum of 203 terms (gamma_202 of the absolute row sums)
    u = unit_roundoff(dtype)
    k = int(np.diff(A.indptr).max()) + 2 + 202
    lim = (k * u / (1 - k * u)) * np.abs(A.data).astype(LD).sum()
    assert abs(LD(float(expr.sum(S).glom())) - A.data.astype(LD).sum()) <= lim
  # pagerank against the same iteration in np.longdouble
  n, T = 500, 5
  Wm = site_graph(n, 6, 0.9, seed=4, tile_hint=(90, n))
  ref = Wm.glom()
  p = np.full((n, 1), LD(1) / n)
  Wl = ref.astype(np.float64)
  for _ in range(T):
    p = LD(np.float32(0.85)) * _ld_dot(Wl, p) + LD(np.float32((1.0 - 0.85) / n))
  got = pagerank(Wm, num_iter=T).glom()
  kmax = int(np.diff(ref.indptr).max())
  assert np.all(np.abs(got.astype(LD) - p) <= 2 * T * (kmax + 4) * unit_roundoff(np.float32) * p)
  # cgit
  A = _spd(200)
  x = np.ones((200, 1))
  z = cgit(expr.from_numpy(A, tile_hint=(70, 200)), x).glom()
  assert np.linalg.norm(A.dot(z) - x) / np.linalg.norm(x) <= 1e-6


def _ld_dot(W, p):
  """W @ p with np.longdouble accumulation (W scipy CSR with exactly representable values)."""
  out = np.zeros((W.shape[0], 1), np.longdouble)
  for i in range(W.shape[0]):
    a, b = W.indptr[i], W.indptr[i + 1]
    out[i, 0] = (W.data[a:b].astype(np.longdouble) * p[W.indices[a:b], 0]).sum()
  return out


def test_layout_independence(gpu_workers):
  """dot at W = 1 and W = 3 gives the same bits: rows never split across slabs
  and every slab runs with the whole matrix's g."""
  from spartan_amd import expr
  A = sparse_data('ragged', 301, 2200, np.float32, lengths=[0, 3, 70, 500, 2100, 9, 1])
  X = dense_data(2200, 3, np.float32)
  out = []
  for W, hint in ((1, None), (3, (40, 2200))):
    gpu_workers(W)
    out.append(expr.dot(expr.from_numpy(A, tile_hint=hint), X).glom())
  assert same_bits(out[0], out[1])
