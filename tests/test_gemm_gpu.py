"""spx_gemm on a real MI355X, kernel by kernel: every case
calls HipBackend.gemm on torch tensors, first asks gemm_plan which kernel and
which instantiation its operands reach and asserts the route it was written
for, then compares every element of C with a reference.

Two kinds of input, two references:

* exact -- integer-valued floats from {-4..4}, C from {-1000..1000}, alpha and
  beta from {1, 2, -1, 0}: every partial sum stays below 2^24 (16 (2 x 8192 +
  3) = 262,192), so any summation order gives the same value in fp32 and fp64
  and the result must EQUAL the reference (a signed zero compares equal to
  zero).  Up to HOST_MACS multiply-adds the reference is NumPy float64 `@` on
  the host; above, a torch fp64 product of the same tensors on the device (a
  checker only, exact for the same reason) at every element, plus NumPy
  float64 `@` on 32 whole rows: the first and last row of the first and last
  block tile, both sides of the 32-, 64- and 128-row wave boundaries, and
  random ones.
* rounded -- oracle.rng uniform [0, 1) values (no cancellation): relative
  error <= 1e-5 (fp32) / 1e-12 (fp64) at every element, against a float64
  product for fp32 (NumPy below HOST_MACS, torch fp64 on the device above)
  and against np.longdouble `@` for fp64 (large shapes: torch fp64 on the
  device at every element, longdouble on sampled rows and columns).

C comes in three forms: (a) beta = 0 into a NaN-filled C, (b) beta = 1 onto
integers / uniform values, (c) beta = 0 into a column-slice view of a wider
NaN-filled buffer that starts at an odd column (ldc > N, base not 16-byte
aligned), after which the buffer outside the view must still be all NaN.
Operands of the bounds-checked instantiations are views into NaN-filled
buffers (a NaN row above and below, NaN columns to the right), so a read past
M, N or K poisons the result.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HOST_MACS = 10 ** 8
RTOL = {np.float32: 1e-5, np.float64: 1e-12}
DTYPES = [np.float32, np.float64]
MODES = {'a': (1.0, 0.0), 'b': (1.0, 1.0), 'c': (1.0, 0.0)}  # C form -> (alpha, beta)
NAN = float('nan')
MAXERR = {}  # (kernel, dtype name) -> largest relative error a rounded case saw


# ------------------------------------------------------------------ helpers
def _tdt(dtype):
  from spartan_amd import backend
  return backend.torch_dtype(dtype)


def _np_dt(t):
  from spartan_amd import backend
  return backend.np_dtype(t.dtype)


def _be(gpu_ctx):
  from spartan_amd import backend
  be = backend.get()
  assert isinstance(be, backend.HipBackend)
  return be


def _plan(A, B):
  """The route of A @ B, asked with the operands' own addresses and strides."""
  from spartan_amd import backend
  return backend.gemm_plan(_np_dt(A), A.shape[0], B.shape[1], A.shape[1], A.data_ptr(), A.stride(0),
                           B.data_ptr(), B.stride(0))


def _probe(dtype, M, N, K=16):
  """The route of a contiguous, 16-byte aligned product (for tile sizes and the flush distance)."""
  from spartan_amd import backend
  return backend.gemm_plan(dtype, M, N, K)


def _routed(A, B, kernel, aligned):
  p = _plan(A, B)
  assert (p['kernel'], p['aligned']) == (kernel, aligned), \
      'this case was written for %s aligned=%s and now reaches %s' % (kernel, aligned, p)
  return p


def _ints(shape, lo, hi, dtype, seed):
  import torch
  g = torch.Generator(device='cuda')
  g.manual_seed(seed)
  return torch.randint(lo, hi + 1, tuple(shape), generator=g, device='cuda').to(_tdt(dtype))


def _uniform(be, shape, seed, dtype):
  """oracle.rng.rand(shape, seed, dtype), made by the device's fill kernel
  (the same generator bit for bit; test_gpu_parity holds the two together)."""
  import torch
  from spartan_amd import backend
  t = torch.empty(tuple(shape), dtype=_tdt(dtype), device='cuda')
  be.fill(t, backend.FILL_UNIFORM, 0.0, 1.0, seed, (0,) * len(shape), tuple(shape))
  return t


def _embed(X, extra, row_pad=1, col0=0):
  """X as a view into a NaN-filled buffer: ``row_pad`` NaN rows above and
  below, rows of X.shape[1] + ``extra`` elements, X starting at column ``col0``."""
  import torch
  M, K = X.shape
  buf = torch.full((M + 2 * row_pad, K + extra), NAN, dtype=X.dtype, device=X.device)
  v = buf[row_pad:row_pad + M, col0:col0 + K]
  v.copy_(X)
  return v


def _loose(X):
  """X for a bounds-checked instantiation: odd leading dimension, NaN all round."""
  return _embed(X, 3, col0=1)


def _c_form(mode, C0):
  """(C, enclosing buffer or None) for one of the three forms of C."""
  import torch
  M, N = C0.shape
  if mode == 'b':
    return C0.clone(), None
  if mode == 'a':
    return torch.full((M, N), NAN, dtype=C0.dtype, device=C0.device), None
  buf = torch.full((M, N + 8), NAN, dtype=C0.dtype, device=C0.device)
  C = buf[:, 3:3 + N]
  assert C.stride(0) > N and C.data_ptr() % 16 != 0
  return C, buf


def _outside_untouched(buf, N):
  import torch
  return bool(torch.isnan(buf[:, :3]).all()) and bool(torch.isnan(buf[:, 3 + N:]).all())


def _bits(t):
  import torch
  t = t.contiguous()
  return t.view(torch.int32 if t.element_size() == 4 else torch.int64)


def _assert_equal(got, want, what):
  ne = got != want  # a NaN in got is a mismatch
  n = int(ne.sum())
  if n:
    i, j = ne.nonzero()[0].tolist()
    raise AssertionError('%s: %d of %d elements differ, the first at C(%d, %d): got %r, want %r'
                         % (what, n, ne.numel(), i, j, got[i, j].item(), want[i, j].item()))


def _host64(t):
  return t.cpu().numpy().astype(np.float64)


def _rows(M, bm, n=32):
  """At most n rows of C for the host check: the first and last row of the
  first and last block tile, both sides of the wave boundaries, random ones."""
  tm = (M + bm - 1) // bm
  rows = {r for r in (0, bm - 1, (tm - 1) * bm, M - 1, 31, 32, 63, 64, 127, 128) if 0 <= r < M}
  g = np.random.default_rng(M)
  while len(rows) < min(n, M):
    rows.add(int(g.integers(M)))
  return sorted(rows)


def _small(A, B):
  return A.shape[0] * A.shape[1] * B.shape[1] <= HOST_MACS


def _product64(A, B):
  """A @ B in float64 as a device tensor: NumPy on the host up to HOST_MACS
  multiply-adds, else torch on the device."""
  import torch
  if _small(A, B):
    return torch.from_numpy(_host64(A) @ _host64(B)).cuda()
  return A.double() @ B.double()


def _check_exact(be, A, B, kernel, aligned, modes='abc', twice=False, ab=None, Bh=None, seed=1, what=''):
  """Exact inputs: C equals the reference at every element, in every form of
  C of ``modes`` (with ``ab``: those (alpha, beta) pairs instead of the
  form's own); ``twice``: a second run gives the same bits."""
  import torch
  p = _routed(A, B, kernel, aligned)
  M, N = A.shape[0], B.shape[1]
  P, rows = _product64(A, B), None
  if not _small(A, B):  # the device product is a checker: whole rows from NumPy on the host as well
    rows = _rows(M, p['bm'])
    P_rows = _host64(A[rows]) @ (_host64(B) if Bh is None else Bh)
  C0 = _ints((M, N), -1000, 1000, _np_dt(A), seed)
  for mode in modes:
    for alpha, beta in (ab or [MODES[mode]]):
      if mode != 'b' and beta != 0:
        continue
      tag = '%s %s (%d, %d, %d) form %s alpha %g beta %g' % (what, kernel, M, N, A.shape[1], mode, alpha, beta)
      C, buf = _c_form(mode, C0)
      be.gemm(A, B, C, alpha, beta)
      want = alpha * P + beta * C0.double()
      _assert_equal(C.double(), want, tag)
      if buf is not None:
        assert _outside_untouched(buf, N), tag + ': wrote outside the view of C'
      if rows is not None:
        want_rows = alpha * P_rows + beta * _host64(C0[rows])
        np.testing.assert_array_equal(_host64(C[rows]), want_rows, err_msg=tag + ' (host rows)')
      if twice:
        C2, _ = _c_form(mode, C0)
        be.gemm(A, B, C2, alpha, beta)
        assert torch.equal(_bits(C), _bits(C2)), tag + ': a second run gave other bits'
  return p, C


def _note(kernel, dtype, err, what):
  key = (kernel, np.dtype(dtype).name)
  MAXERR[key] = max(MAXERR.get(key, 0.0), err)
  print('gemm max rel err %-9s %-7s %.3e  %s' % (kernel, np.dtype(dtype).name, err, what))


def _check_rounded(be, A, B, kernel, aligned, cases, seed=5, what='', twice=False):
  """Rounded inputs (non-negative): |C - ref| <= rtol (|alpha| A B + |beta| C0)
  at every element, for every (form of C, alpha, beta) of ``cases``."""
  import torch
  dtype = _np_dt(A)
  p = _routed(A, B, kernel, aligned)
  M, K = A.shape
  N = B.shape[1]
  rtol = RTOL[np.dtype(dtype).type]
  small = _small(A, B)
  C0 = _uniform(be, (M, N), seed, dtype)
  if dtype == np.float64 and small:
    ld = np.longdouble
    P = A.cpu().numpy().astype(ld) @ B.cpu().numpy().astype(ld)
    C0h = C0.cpu().numpy().astype(ld)
  else:
    P = _product64(A, B)
    if dtype == np.float64:  # the device product is a checker: sampled rows and columns in longdouble as well
      ld = np.longdouble
      g = np.random.default_rng(K)
      ri, ci = sorted({M - 1, int(g.integers(M))}), sorted({N - 1, int(g.integers(N))})
      Ah, Bh = A.cpu().numpy(), B.cpu().numpy()
      P_r = Ah[ri].astype(ld) @ Bh.astype(ld)
      P_c = Ah.astype(ld) @ Bh[:, ci].astype(ld)
  for mode, alpha, beta in cases:
    tag = '%s %s (%d, %d, %d) form %s alpha %g beta %g' % (what, kernel, M, N, K, mode, alpha, beta)
    C, buf = _c_form(mode, C0)
    be.gemm(A, B, C, alpha, beta)
    if buf is not None:
      assert _outside_untouched(buf, N), tag + ': wrote outside the view of C'
    if dtype == np.float64 and small:
      got = C.cpu().numpy().astype(ld)
      rel = np.abs(got - (alpha * P + beta * C0h)) / (abs(alpha) * P + abs(beta) * C0h)
      assert not np.isnan(rel).any(), tag
      err = float(rel.max())
    else:
      rel = (C.double() - (alpha * P + beta * C0.double())).abs() / (abs(alpha) * P + abs(beta) * C0.double())
      assert not bool(torch.isnan(rel).any()), tag
      err = float(rel.max())
      if dtype == np.float64:
        Ch, C0s = C.cpu().numpy(), C0.cpu().numpy()
        for got, ref, c0 in ((Ch[ri], P_r, C0s[ri]), (Ch[:, ci], P_c, C0s[:, ci])):
          r = np.abs(got.astype(ld) - (alpha * ref + beta * c0.astype(ld))) / (abs(alpha) * ref + abs(beta) * c0)
          err = max(err, float(r.max()))
    _note(kernel, dtype, err, tag)
    assert err <= rtol, '%s: max rel err %.3e above %g' % (tag, err, rtol)
    if twice:
      C2, _ = _c_form(mode, C0)
      be.gemm(A, B, C2, alpha, beta)
      assert torch.equal(_bits(C), _bits(C2)), tag + ': a second run gave other bits'
  return p


# ----------------------------------------------------------------- fixtures
M_P3, N_P3, N_BIG = 4096, 8192, 8320   # 16 x 32 big tiles; N_BIG % 256 == 128: whole 256 x 128 tiles only


def _kspec(fk, bk, spec):
  """K of a (flushes, K-tiles, tail) triple for a kernel that flushes every fk and stages bk."""
  return spec[0] * fk + spec[1] * bk + spec[2]


@pytest.fixture(scope='module')
def shapes(gpu_ctx):
  """Today's tile sizes and flush distance, from the library."""
  s = {'small': _probe(np.float32, 128, 128), 'big': _probe(np.float32, M_P3, N_BIG),
       'p3': _probe(np.float32, M_P3, N_P3), 'f64': _probe(np.float64, 128, 128)}
  assert [s[k]['kernel'] for k in ('small', 'big', 'p3', 'f64')] == ['F32_SMALL', 'F32_BIG', 'F32_P3', 'F64'], s
  assert s['small']['flush_k'] == s['big']['flush_k'] == s['p3']['flush_k'] > 0 and s['f64']['flush_k'] == 0
  s['fk'], s['bk'] = s['p3']['flush_k'], s['p3']['bk']
  s['kmax'] = s['fk'] + 3 * s['bk']
  return s


@pytest.fixture(scope='module')
def exact_big(gpu_ctx, shapes):
  """Exact operands at the largest K, A (M_P3, kmax) and B (kmax, N_BIG) in
  fp32, with B on the host in float64; the cases take prefix views."""
  import torch
  A = _ints((M_P3, shapes['kmax']), -4, 4, np.float32, 101)
  B = _ints((shapes['kmax'], N_BIG), -4, 4, np.float32, 102)
  d = {'A': A, 'B': B, 'Bh': _host64(B)}
  yield d
  d.clear()
  del A, B
  torch.cuda.empty_cache()


@pytest.fixture(scope='module')
def rounded_big(gpu_ctx, shapes):
  """Uniform [0, 1) operands of the same sizes, fp32."""
  import torch
  from oracle import rng
  be = _be(gpu_ctx)
  kmax = shapes['kmax']
  A = _uniform(be, (M_P3, kmax), 201, np.float32)
  B = _uniform(be, (kmax, N_BIG), 202, np.float32)
  k = np.arange(kmax, dtype=np.uint64)  # the device's values are oracle.rng's: one row of A, one column of B
  np.testing.assert_array_equal(A[77].cpu().numpy(), rng.uniform_values(np.uint64(77 * kmax) + k, 201, 0.0, 1.0,
                                                                        np.float32))
  np.testing.assert_array_equal(B[:, 5].cpu().numpy(), rng.uniform_values(k * np.uint64(N_BIG) + np.uint64(5), 202,
                                                                          0.0, 1.0, np.float32))
  d = {'A': A, 'B': B}
  yield d
  d.clear()
  del A, B
  torch.cuda.empty_cache()


@pytest.fixture(scope='module', autouse=True)
def report():
  yield
  for (kernel, dt), err in sorted(MAXERR.items()):
    print('gemm max rel err over the rounded cases: %-9s %-7s %.3e' % (kernel, dt, err))


def _exact_pair(M, N, K, dtype, seed, loose):
  A = _ints((M, K), -4, 4, dtype, seed)
  B = _ints((K, N), -4, 4, dtype, seed + 1)
  return (_loose(A), _loose(B)) if loose else (A, B)


# ------------------------------------------- Small fp32 and GemmF64: edges
EDGE_SHAPES = [(1, 1, 1), (33, 65, 17), (127, 129, 15), (128, 128, 16), (129, 127, 17), (300, 257, 40)]


@pytest.mark.parametrize('M,N,K', EDGE_SHAPES)
@pytest.mark.parametrize('dtype', DTYPES)
def test_edge_tiles_exact(gpu_ctx, shapes, dtype, M, N, K):
  """Edge tiles of the 128 x 128 x 16 kernels in every form of C; (128, 128,
  16) contiguous takes the instantiation without bounds checks."""
  be = _be(gpu_ctx)
  t = shapes['small' if dtype == np.float32 else 'f64']
  aligned = M % t['bm'] == 0 and N % t['bn'] == 0 and K % t['bk'] == 0
  A, B = _exact_pair(M, N, K, dtype, 11 * M + N, loose=not aligned)
  _check_exact(be, A, B, 'F32_SMALL' if dtype == np.float32 else 'F64', aligned)


@pytest.mark.parametrize('mt', [11, 10])
@pytest.mark.parametrize('dtype', DTYPES)
def test_tile_map_exact(gpu_ctx, shapes, dtype, mt):
  """The block -> tile map where it is irregular: (11 bm + 5, 3 bn + 1, 19)
  -- 12 x 4 tiles, a last group of 4 tile rows -- and (10 bm + 5, 3 bn + 1,
  19) -- 11 x 4 = 44 tiles, ntiles % 8 == 4 (the XCD ranges differ in
  length) and a last group of 3 tile rows; a tile written twice or not at
  all shows in form (b).  fp64 runs the same shapes ungrouped."""
  be = _be(gpu_ctx)
  t = shapes['small' if dtype == np.float32 else 'f64']
  M, N, K = mt * t['bm'] + 5, 3 * t['bn'] + 1, 19
  tiles_m, tiles_n = -(-M // t['bm']), -(-N // t['bn'])
  assert tiles_m % 8 != 0 and (mt != 10 or (tiles_m % 8, (tiles_m * tiles_n) % 8) == (3, 4))
  A, B = _exact_pair(M, N, K, dtype, 7 + mt, loose=True)
  _check_exact(be, A, B, 'F32_SMALL' if dtype == np.float32 else 'F64', False, modes='b')


# ---------------------------------------------------------- Small: flushes
FLUSH_K = [(1, 0, 0), (1, 1, 0), (1, 0, -1), (1, 0, 1), (1, 1, 5), (2, 0, 3)]  # 8192, 8208; 8191, 8193, 8213, 16387


@pytest.mark.parametrize('spec', FLUSH_K, ids=lambda s: 'K=%dfk%+dbk%+d' % s)
@pytest.mark.parametrize('kind', ['exact', 'rounded'])
def test_small_flush(gpu_ctx, shapes, kind, spec):
  """The flush of the accumulators into C every flush_k of K in the fp32
  128 x 128 kernel: none at exactly flush_k, one with a whole K-tile or a K
  tail after it, two with a tail; (bm, bn, K) without bounds checks for K a
  multiple of bk, else (130, 70, K) with edge tiles.  Forms (a) and (b),
  twice: the atomics are deterministic."""
  from oracle import rng
  be = _be(gpu_ctx)
  t = shapes['small']
  K = _kspec(t['flush_k'], t['bk'], spec)
  aligned = K % t['bk'] == 0
  M, N = (t['bm'], t['bn']) if aligned else (130, 70)
  if kind == 'exact':
    A, B = _exact_pair(M, N, K, np.float32, K, loose=not aligned)
    _check_exact(be, A, B, 'F32_SMALL', aligned, modes='ab', twice=True)
  else:
    import torch
    A = torch.as_tensor(rng.rand((M, K), 21, np.float32)).cuda()
    B = torch.as_tensor(rng.rand((K, N), 22, np.float32)).cuda()
    if not aligned:
      A, B = _loose(A), _loose(B)
    _check_rounded(be, A, B, 'F32_SMALL', aligned, [('a', 1.0, 0.0), ('b', 1.0, 1.0)], twice=True)


# -------------------------------------------------------------- fp32 Big
@pytest.mark.parametrize('M,N,K', [(4093, 8187, 19), (4861, 6913, 19), (1, 130817, 33)])
def test_big_bounds_checked_exact(gpu_ctx, M, N, K):
  """GemmF32Big with edge tiles: 16 x 32 = 512 big tiles exactly; 19 x 55
  tiles of 256 x 128 (a last group of 3 tile rows, ntiles % 8 == 5); one row."""
  be = _be(gpu_ctx)
  A, B = _exact_pair(M, N, K, np.float32, M, loose=True)
  p, _ = _check_exact(be, A, B, 'F32_BIG', False)
  if M == 4861:
    tiles_m, tiles_n = -(-M // p['bm']), -(-N // p['bn'])
    assert tiles_m % 8 == 3 and (tiles_m * tiles_n) % 8 != 0


def test_big_flush_k_tail(gpu_ctx, shapes, exact_big, rounded_big):
  """GemmF32Big, edge tiles, one flush and a K tail: (4093, 8187, flush_k + bk + 1), exact and rounded."""
  be = _be(gpu_ctx)
  K = shapes['fk'] + shapes['bk'] + 1
  A, B = exact_big['A'][:4093, :K], exact_big['B'][:K, :8187]
  _check_exact(be, A, B, 'F32_BIG', False, Bh=exact_big['Bh'][:K, :8187])
  A, B = rounded_big['A'][:4093, :K], rounded_big['B'][:K, :8187]
  _check_rounded(be, A, B, 'F32_BIG', False, [('a', 1.0, 0.0), ('b', 1.0, 1.0), ('c', 1.0, 0.0)])


@pytest.mark.parametrize('spec', [(0, 1, 0), (1, 1, 0)], ids=lambda s: 'K=%dfk%+dbk%+d' % s)
def test_big_aligned_exact(gpu_ctx, shapes, exact_big, spec):
  """GemmF32Big without bounds checks: N % 256 == 128, K = bk and flush_k + bk."""
  be = _be(gpu_ctx)
  K = _kspec(shapes['fk'], shapes['bk'], spec)
  A, B = exact_big['A'][:, :K], exact_big['B'][:K, :]
  _check_exact(be, A, B, 'F32_BIG', True, Bh=exact_big['Bh'][:K])


# ---------------------------------------------------------------- fp32 p3
P3_K = [(0, 1, 0), (0, 2, 0), (0, 3, 0), (0, 4, 0), (0, 5, 0), (1, 0, 0), (1, 1, 0), (1, 2, 0), (1, 3, 0)]


@pytest.mark.parametrize('spec', P3_K, ids=lambda s: 'K=%dfk%+dbk%+d' % s)
def test_p3_exact(gpu_ctx, shapes, exact_big, spec):
  """gemm_f32_p3 at 1 to 5 K-tiles (the pipeline fill, the odd / even tail of
  its two-tile loop) and at a whole flush chunk followed by 0 to 3 K-tiles,
  in every form of C, twice.  A and B are prefix views of the operands of the
  largest K: lda stays kmax, and the route must still be the p3 kernel."""
  be = _be(gpu_ctx)
  K = _kspec(shapes['fk'], shapes['bk'], spec)
  A, B = exact_big['A'][:, :K], exact_big['B'][:K, :N_P3]
  assert A.stride(0) == shapes['kmax'] and B.stride(0) == N_BIG
  _check_exact(be, A, B, 'F32_P3', True, twice=True, Bh=exact_big['Bh'][:K, :N_P3])


def test_p3_tile_map_exact(gpu_ctx):
  """gemm_f32_p3 at 3 x 171 = 513 tiles: a single, partial group of 3 tile rows and ntiles % 8 == 1."""
  be = _be(gpu_ctx)
  A, B = _exact_pair(768, 43776, 48, np.float32, 31, loose=False)
  p, _ = _check_exact(be, A, B, 'F32_P3', True, twice=True)
  tiles_m, tiles_n = 768 // p['bm'], 43776 // p['bn']
  assert tiles_m % 8 == 3 and (tiles_m * tiles_n) % 8 == 1


def test_p3_rounded_and_against_big(gpu_ctx, shapes, rounded_big):
  """gemm_f32_p3 on rounded inputs at K = flush_k + 3 bk, and the claim of
  spx.hip that the p3 and the two-stage kernels form the same chains: the
  first N_P3 columns of the (M_P3, N_BIG, flush_k + bk) Big product equal the
  (M_P3, N_P3, flush_k + bk) p3 product bit for bit."""
  import torch
  be = _be(gpu_ctx)
  A, B = rounded_big['A'], rounded_big['B'][:, :N_P3]
  _check_rounded(be, A, B, 'F32_P3', True, [('a', 1.0, 0.0), ('b', 1.0, 1.0), ('c', 1.0, 0.0)], twice=True)
  K = shapes['fk'] + shapes['bk']
  A, Bw = rounded_big['A'][:, :K], rounded_big['B'][:K]
  _check_rounded(be, A, Bw, 'F32_BIG', True, [('a', 1.0, 0.0)])
  _check_rounded(be, A, Bw[:, :N_P3], 'F32_P3', True, [('a', 1.0, 0.0)])
  Cb = torch.full((M_P3, N_BIG), NAN, dtype=torch.float32, device='cuda')
  Cp = torch.full((M_P3, N_P3), NAN, dtype=torch.float32, device='cuda')
  be.gemm(A, Bw, Cb)
  be.gemm(A, Bw[:, :N_P3], Cp)
  assert torch.equal(_bits(Cb[:, :N_P3]), _bits(Cp)), 'the p3 and the two-stage kernel round differently'


# ------------------------------------------------- fp64 at >= 1024 tiles
@pytest.mark.parametrize('case', ['K=bk', 'K=fk+bk', 'edges'])
def test_f64_many_tiles(gpu_ctx, shapes, exact_big, case):
  """fp64 where the experimental three-stage kernel would be routed (>= 1024
  tiles): today GemmF64, and the route assertion says so.  Exact in every
  form of C; K = flush_k + bk also rounded."""
  be = _be(gpu_ctx)
  if case == 'edges':
    A, B = _exact_pair(4093, 4091, 19, np.float64, 41, loose=True)
    _check_exact(be, A, B, 'F64', False)
    return
  K = shapes['bk'] if case == 'K=bk' else shapes['fk'] + shapes['bk']
  A, B = exact_big['A'][:, :K].double(), exact_big['B'][:K, :4096].double()
  assert _probe(np.float64, 4096, 4096, K)['kernel'] == 'F64'
  _check_exact(be, A, B, 'F64', True, Bh=exact_big['Bh'][:K, :4096])
  if case != 'K=bk':
    del A, B
    A, B = _uniform(be, (4096, K), 301, np.float64), _uniform(be, (K, 4096), 302, np.float64)
    _check_rounded(be, A, B, 'F64', True, [('a', 1.0, 0.0), ('b', 1.0, 1.0)])


# ------------------------------------------- operand strides and bases
@pytest.mark.parametrize('M,N,kernel', [(128, 128, 'small'), (M_P3, N_BIG, 'big'), (M_P3, N_P3, 'p3')])
@pytest.mark.parametrize('dtype', DTYPES)
def test_operand_strides_and_bases(gpu_ctx, shapes, dtype, M, N, kernel):
  """A and B as views into wider NaN-filled buffers.  Rows padded by four
  elements keep the instantiation without bounds checks (and the p3 kernel);
  a row padded by one, or an operand that starts one element into its buffer,
  must select the bounds-checked one (p3 becomes Big) -- and the result must
  not change."""
  import torch
  be = _be(gpu_ctx)
  K = shapes['bk']
  want = {'small': 'F32_SMALL', 'big': 'F32_BIG', 'p3': 'F32_P3'}[kernel] if dtype == np.float32 else 'F64'
  loose = 'F32_BIG' if want == 'F32_P3' else want
  A0, B0 = _exact_pair(M, N, K, dtype, 51, loose=False)
  _routed(A0, B0, want, True)
  results = []
  for a_extra, a_col, b_extra, b_col, kern, aligned in [
      (4, 0, 4, 0, want, True),     # lda = K + 4, ldb = N + 4
      (4, 4, 4, 4, want, True),     # and starting 16 bytes into the row
      (1, 0, 4, 0, loose, False),   # lda = K + 1
      (4, 0, 1, 0, loose, False),   # ldb = N + 1
      (4, 1, 4, 0, loose, False),   # A starts one element into its buffer
      (4, 0, 4, 1, loose, False)]:  # B does
    if dtype == np.float64 and (a_col == 4 or b_col == 4):
      a_col, b_col = a_col // 2, b_col // 2  # 16 bytes are two doubles
    A, B = _embed(A0, a_extra, col0=a_col), _embed(B0, b_extra, col0=b_col)
    assert A.stride(0) == K + a_extra and B.stride(0) == N + b_extra
    what = 'lda K%+d ldb N%+d A at +%d B at +%d' % (a_extra, b_extra, a_col, b_col)
    results.append(_check_exact(be, A, B, kern, aligned, modes='a', what=what)[1])
  for C in results[1:]:
    assert torch.equal(_bits(C), _bits(results[0]))


# -------------------------------------------------------- alpha and beta
EXACT_AB = [(a, b) for a in (1.0, 2.0, -1.0, 0.0) for b in (1.0, 2.0, -1.0, 0.0)]
ROUNDED_AB = [(-0.5, 0.0), (1.0, 0.75), (2.5, -1.25)]


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('flush', [False, True])
def test_scaling_exact(gpu_ctx, shapes, dtype, flush):
  """alpha and beta from {1, 2, -1, 0}: scaling stays exact, with edge tiles, without and with flushes."""
  be = _be(gpu_ctx)
  K = shapes['fk'] + 21 if flush else 17
  A, B = _exact_pair(130, 70, K, dtype, 61, loose=True)
  _check_exact(be, A, B, 'F32_SMALL' if dtype == np.float32 else 'F64', False, modes='b', ab=EXACT_AB)


@pytest.mark.parametrize('flush', [False, True])
@pytest.mark.parametrize('kernel', ['F32_SMALL', 'F32_BIG', 'F32_P3', 'F64'])
def test_scaling_rounded(gpu_ctx, shapes, rounded_big, kernel, flush):
  """alpha != 1 and beta outside {0, 1} (for fp32: the row-scaling kernel,
  then the GEMM with beta = 1) on every float kernel at a small shape of its
  own, one K-tile and a tail or one flush and a tail; the tolerance relative
  to |alpha| |A| |B| + |beta| |C|."""
  import torch
  from oracle import rng
  be = _be(gpu_ctx)
  fk, bk = shapes['fk'], shapes['bk']
  cases = [('a' if beta == 0 else 'b', alpha, beta) for alpha, beta in ROUNDED_AB]
  if kernel in ('F32_SMALL', 'F64'):
    dtype = np.float32 if kernel == 'F32_SMALL' else np.float64
    M, N, K = (130, 70, fk + 21 if flush else 33) if dtype == np.float32 else (33, 65, fk + 21 if flush else 17)
    A = _loose(torch.as_tensor(rng.rand((M, K), 71, dtype)).cuda())
    B = _loose(torch.as_tensor(rng.rand((K, N), 72, dtype)).cuda())
    _check_rounded(be, A, B, kernel, False, cases)
  elif kernel == 'F32_BIG':
    K = fk + bk + 1 if flush else bk + 3
    _check_rounded(be, rounded_big['A'][:4093, :K], rounded_big['B'][:K, :8187], kernel, False, cases)
  else:
    K = fk + bk if flush else bk
    _check_rounded(be, rounded_big['A'][:, :K], rounded_big['B'][:K, :N_P3], kernel, True, cases)


# ----------------------------------------------------------------- integer
@pytest.mark.parametrize('M,N,K', [(1, 1, 1), (15, 17, 16), (16, 16, 17), (33, 50, 100)])
@pytest.mark.parametrize('dtype', [np.int32, np.int64])
def test_integer_wraps(gpu_ctx, dtype, M, N, K):
  """Integer GEMM at full-range values: every sum wraps, and the result is
  NumPy's wrapping `@` in unsigned arithmetic of the same width, with alpha
  and beta, into a C view with ldc > N whose surroundings stay as they were."""
  import torch
  be = _be(gpu_ctx)
  udt = np.uint32 if dtype == np.int32 else np.uint64
  info = np.iinfo(dtype)
  g = np.random.default_rng(M * 1000 + N)
  Ah, Bh, C0h = (g.integers(info.min, info.max, size=s, dtype=dtype, endpoint=True) for s in ((M, K), (K, N), (M, N)))
  A, B = torch.as_tensor(Ah).cuda(), torch.as_tensor(Bh).cuda()
  assert _routed(A, B, 'INT', False)['flush_k'] == 0
  for alpha, beta in [(1, 0), (3, -2)]:
    with np.errstate(over='ignore'):
      want = udt(alpha & int(np.iinfo(udt).max)) * (Ah.view(udt) @ Bh.view(udt))
      if beta:
        want = want + udt(beta & int(np.iinfo(udt).max)) * C0h.view(udt)
    buf = torch.full((M, N + 5), 77, dtype=A.dtype, device='cuda')
    C = buf[:, 2:2 + N]
    C.copy_(torch.as_tensor(C0h).cuda())
    be.gemm(A, B, C, alpha, beta)
    np.testing.assert_array_equal(C.cpu().numpy().view(udt), want, err_msg='alpha %d beta %d' % (alpha, beta))
    assert bool((buf[:, :2] == 77).all()) and bool((buf[:, 2 + N:] == 77).all())


# ------------------------------------------------------- argument contract
@pytest.mark.parametrize('dtype', [np.float32, np.float64, np.int64])
def test_argument_contract(gpu_ctx, dtype):
  """K == 0 is ENOTSUP and leaves C untouched; M == 0 or N == 0 is OK and
  writes nothing; lda < K is EINVAL -- checked before any launch."""
  import torch
  from spartan_amd import backend
  be = _be(gpu_ctx)
  dt = backend.spx_dtype(dtype)
  fill = NAN if np.dtype(dtype).kind == 'f' else -12345
  A = torch.ones((8, 8), dtype=_tdt(dtype), device='cuda')
  B = torch.ones((8, 8), dtype=_tdt(dtype), device='cuda')
  C = torch.full((8, 8), fill, dtype=_tdt(dtype), device='cuda')
  before = _bits(C).clone() if np.dtype(dtype).kind == 'f' else C.clone()

  def call(M, N, K, lda=8, ldb=8, ldc=8):
    import ctypes
    return be.lib.spx_gemm(dt, M, N, K, ctypes.c_void_p(A.data_ptr()), lda, ctypes.c_void_p(B.data_ptr()), ldb,
                           ctypes.c_void_p(C.data_ptr()), ldc, 1.0, 0.0, backend.current_stream())

  def untouched():
    torch.cuda.synchronize()
    return torch.equal(_bits(C) if np.dtype(dtype).kind == 'f' else C, before)

  assert call(8, 8, 0) == -3 and b'K == 0' in be.lib.spx_last_error() and untouched()
  assert call(0, 8, 8) == 0 and call(8, 0, 8) == 0 and call(0, 0, 0) == 0 and untouched()
  assert call(8, 8, 8, lda=7) == -1 and b'leading dimension' in be.lib.spx_last_error() and untouched()
  assert call(8, 8, 8, ldc=7) == -1 and untouched()
  assert call(8, 8, 8) == 0 and not untouched()
