"""GPU parity: spartan_amd (libspx.so + generated gfx950 kernels) vs the oracle.

Shapes and expectations restate the reference's own hot-path tests
(tests/test_reduce.py, test_dot.py, test_matmul.py, test_maptiles.py) plus
the BASELINE configs at oracle-friendly sizes.  Tolerances (BASELINE.json
north_star): integer / index results bit-exact; fp32 1e-5 relative, fp64
1e-12 relative -- for reductions either within that of the reference CPU
result, or at least as close to the exact (fp64-accumulated) value as the
reference CPU result is.
"""
import os
import sys

import zlib

import numpy as np
import pytest

from oracle import rng
from oracle import spartan_cpu as O

HERE = os.path.dirname(os.path.abspath(__file__))

pytestmark = pytest.mark.gpu

TEST_SIZE = 50
WORKERS = [1, 3]


def check_fp(gpu, cpu, exact, rtol, cond=None):
  """Every element within rtol of the CPU result, or at least as close to the
  fp64-exact value as the CPU result is.  ``cond`` (sum of |terms| per
  element, for sums with cancellation): an element also passes when its
  error is within rtol * 1e-2 of its condition -- 1e-7 (fp32) / 1e-14 (fp64)
  of sum |terms|, tighter than the typical error of an fp32 / fp64 sum of a
  few hundred terms -- since a result near zero makes 'relative to the
  result' a test of luck (which of two roundings of a cancelled sum landed
  closer), not of accuracy.

  Returns (n_cond, ratio): how many elements passed ONLY by the ``cond``
  rule, and the maximum over all elements of the error beyond the rounding of
  the result to its own dtype, (|gpu - exact| - ulp(exact) / 2) / cond (0
  without ``cond``), so a caller can bound both (round-6 verdict)."""
  gdt = np.asarray(gpu).dtype
  half_ulp = (0.5 * np.spacing(np.abs(np.asarray(exact, dtype=np.float64)).astype(gdt)).astype(np.float64)
              if gdt.kind == 'f' else 0.0)
  gpu, cpu, exact = (np.asarray(v, dtype=np.float64) for v in (gpu, cpu, exact))
  assert gpu.shape == cpu.shape
  scale = np.maximum(np.abs(cpu), 1e-30)
  close = np.abs(gpu - cpu) <= rtol * scale
  better = np.abs(gpu - exact) <= np.abs(cpu - exact) + rtol * 1e-3 * scale
  strict = close | better
  n_cond, ratio = 0, 0.0
  if cond is not None:
    cond = np.maximum(np.asarray(cond, dtype=np.float64), 1e-300)
    by_cond = np.abs(gpu - exact) <= rtol * 1e-2 * cond
    n_cond = int((by_cond & ~strict).sum())
    ratio = float((np.maximum(np.abs(gpu - exact) - half_ulp, 0.0) / cond).max()) if gpu.size else 0.0
    strict = strict | by_cond
  bad = ~strict
  assert not bad.any(), 'max rel err %g at %s' % (
      (np.abs(gpu - cpu) / scale).max(), np.argwhere(bad)[:5])
  return n_cond, ratio


@pytest.fixture
def ex(gpu_workers):
  from spartan_amd import expr
  return expr, gpu_workers


# ------------------------------------------------------------ reduce KATs
@pytest.mark.parametrize('W', WORKERS)
def test_sum_3d(ex, W):
  expr, setw = ex
  setw(W)
  x = expr.arange((TEST_SIZE,) * 3, dtype=np.int64)
  nx = np.arange(TEST_SIZE ** 3, dtype=np.int64).reshape((TEST_SIZE,) * 3)
  for axis in [None, 0, 1, 2]:
    got = x.sum(axis).glom()
    np.testing.assert_array_equal(got, nx.sum(axis))
    np.testing.assert_array_equal(got, O.sum_tiles(nx, axis, W))


@pytest.mark.parametrize('W', WORKERS)
def test_sum_2d_1d(ex, W):
  expr, setw = ex
  setw(W)
  x = expr.arange((TEST_SIZE, TEST_SIZE), dtype=np.int64)
  nx = np.arange(TEST_SIZE * TEST_SIZE, dtype=np.int64).reshape((TEST_SIZE, TEST_SIZE))
  for axis in [None, 0, 1]:
    np.testing.assert_array_equal(x.sum(axis).glom(), nx.sum(axis))
  y = expr.arange((TEST_SIZE,), dtype=np.int64)
  np.testing.assert_array_equal(y.sum().glom(), np.arange(TEST_SIZE).sum())


@pytest.mark.parametrize('W', WORKERS)
@pytest.mark.parametrize('kind', ['argmin', 'argmax'])
def test_arg_3d(ex, W, kind):
  expr, setw = ex
  setw(W)
  x = expr.arange((TEST_SIZE,) * 3, dtype=np.int64)
  nx = np.arange(TEST_SIZE ** 3, dtype=np.int64).reshape((TEST_SIZE,) * 3)
  for axis in [None, 0, 1, 2]:
    got = getattr(x, kind)(axis).glom()
    np.testing.assert_array_equal(got, getattr(nx, kind)(axis))
    np.testing.assert_array_equal(got, O.arg_tiles(nx, axis, W, kind))


@pytest.mark.parametrize('W', WORKERS)
def test_arg_1d_2d(ex, W):
  expr, setw = ex
  setw(W)
  x = expr.arange((TEST_SIZE,), dtype=np.int64)
  assert x.argmin().glom() == 0 and x.argmax().glom() == TEST_SIZE - 1
  y = expr.arange((TEST_SIZE, TEST_SIZE), dtype=np.int64)
  ny = np.arange(TEST_SIZE * TEST_SIZE).reshape(TEST_SIZE, TEST_SIZE)
  np.testing.assert_array_equal(expr.glom(y.argmin(axis=1)), ny.argmin(axis=1))
  np.testing.assert_array_equal(expr.glom(y.argmax(axis=1)), ny.argmax(axis=1))


@pytest.mark.parametrize('W', WORKERS)
def test_simple_sum_and_counts(ex, W):
  expr, setw = ex
  setw(W)
  for axis in [0, 1, None]:
    a = expr.ones((TEST_SIZE, TEST_SIZE)) + expr.ones((TEST_SIZE, TEST_SIZE))
    np.testing.assert_array_equal(a.sum(axis=axis).glom(), 2 * np.ones((TEST_SIZE, TEST_SIZE)).sum(axis))
  assert expr.count_nonzero(expr.ones((TEST_SIZE,))).glom() == TEST_SIZE
  assert expr.count_nonzero(expr.zeros((TEST_SIZE,))).glom() == 0
  assert expr.count_zero(expr.ones((TEST_SIZE,))).glom() == 0
  assert expr.count_zero(expr.zeros((TEST_SIZE,))).glom() == TEST_SIZE


# ------------------------------------------------------------------ maps
@pytest.mark.parametrize('W', WORKERS)
def test_maptiles(ex, W):
  expr, setw = ex
  setw(W)
  a, b = expr.ones((20, 20)), expr.ones((20, 20))
  np.testing.assert_array_equal((a + b).glom(), 2 * np.ones((20, 20)))
  c = expr.ones((10, 10))
  np.testing.assert_array_equal((a[0:10, 0:10] if False else c + c + c).glom(), 3 * np.ones((10, 10)))
  many = expr.ones((10, 10))
  m2 = expr.ones((10, 10))
  s = many + m2 + many + m2 + many + m2 + many + m2 + many + m2
  np.testing.assert_array_equal(s.glom(), 10 * np.ones((10, 10)))
  l = 1.0 + expr.ones((100,), dtype=np.float32)
  got = expr.ln(l).glom()
  assert got.dtype == np.float32
  np.testing.assert_allclose(got, np.log(1.0 + np.ones(100, np.float32)), rtol=1e-6)
  d1, d2 = expr.ones((2, 1)), expr.ones((2, 5))
  np.testing.assert_array_equal((d1 / d2).glom(), np.ones((2, 5)))
  np.testing.assert_array_equal((d2 / d1).glom(), np.ones((2, 5)))


@pytest.mark.parametrize('W', [1, 2, 3])
def test_broadcast_and_scalars(ex, W):
  expr, setw = ex
  setw(W)
  n = np.arange(24.0).reshape(4, 6)
  x = expr.from_numpy(n)
  row = expr.from_numpy(np.arange(6.0).reshape(1, 6))
  col = expr.from_numpy(np.arange(4.0).reshape(4, 1))
  np.testing.assert_array_equal((x + row).glom(), n + np.arange(6.0).reshape(1, 6))
  np.testing.assert_array_equal((x * col - 2).glom(), n * np.arange(4.0).reshape(4, 1) - 2)
  np.testing.assert_array_equal(expr.maximum(x, 7.5).glom(), np.maximum(n, 7.5))
  np.testing.assert_array_equal(((x - row) * col).sum(axis=0).glom(),
                                ((n - np.arange(6.0)) * np.arange(4.0).reshape(4, 1)).sum(0))


def test_lambda_map_traced(ex):
  expr, setw = ex
  setw(2)
  n = np.arange(12.0).reshape(3, 4)
  x = expr.from_numpy(n)
  got = expr.map(x, lambda v: np.sqrt(v) * 2 + 1).glom()
  np.testing.assert_allclose(got, np.sqrt(n) * 2 + 1, rtol=1e-15)


# ------------------------------------------------------------------- dot
@pytest.mark.parametrize('W', WORKERS)
def test_dot_kats(ex, W):
  expr, setw = ex
  setw(W)
  for (m, k, n) in [(132, 100, 77), (67, 100, 77)]:
    av, bv = expr.arange((m, k)), expr.arange((k, n))
    na, nb = np.arange(m * k).reshape(m, k), np.arange(k * n).reshape(k, n)
    got = expr.dot(av, bv).glom()
    np.testing.assert_array_equal(got, np.dot(na, nb))
    np.testing.assert_array_equal(got, O.dot_tiles(na.astype(np.float64), nb.astype(np.float64), W))
  cv, dv = expr.arange((77, 100)), np.arange(8800).reshape(100, 88)
  np.testing.assert_array_equal(expr.dot(cv, dv).glom(), np.dot(np.arange(7700).reshape(77, 100), dv))


@pytest.mark.parametrize('W', WORKERS)
def test_dot_vectors(ex, W):
  expr, setw = ex
  setw(W)
  av, bv = expr.arange(stop=100), expr.arange(stop=100)
  np.testing.assert_array_equal(expr.dot(av, bv).glom(), np.dot(np.arange(100), np.arange(100)))
  for (m, k) in [(100, 77), (77, 100)]:
    a2, b1 = expr.arange((m, k)), expr.arange(stop=k)
    np.testing.assert_array_equal(expr.dot(a2, b1).glom(), np.dot(np.arange(m * k).reshape(m, k), np.arange(k)))
  np.testing.assert_array_equal(expr.dot(expr.arange(stop=100), np.arange(100)).glom(),
                                np.dot(np.arange(100), np.arange(100)))
  np.testing.assert_array_equal(expr.dot(expr.arange((77, 100)), np.arange(100)).glom(),
                                np.dot(np.arange(7700).reshape(77, 100), np.arange(100)))
  with pytest.raises(ValueError):
    expr.dot(expr.arange((3, 4)), expr.arange((5, 2)))


@pytest.mark.parametrize('W', WORKERS)
def test_matmul_int_and_f64(ex, W):
  expr, setw = ex
  setw(W)
  x = expr.arange((100, 50), dtype=np.int64).astype(np.float64)
  y = expr.arange((50, 100), dtype=np.int64).astype(np.float64)
  nx = np.arange(5000, dtype=np.int64).reshape(100, 50).astype(np.float64)
  ny = np.arange(5000, dtype=np.int64).reshape(50, 100).astype(np.float64)
  np.testing.assert_array_equal(expr.dot(x, y).glom(), np.dot(nx, ny))


@pytest.mark.parametrize('dtype,rtol', [(np.float32, 1e-5), (np.float64, 1e-12)])
@pytest.mark.parametrize('shape', [(256, 192, 160), (512, 512, 512), (130, 70, 33)])
@pytest.mark.parametrize('W', [1, 4])
def test_gemm_random(ex, dtype, rtol, shape, W):
  expr, setw = ex
  setw(W)
  m, k, n = shape
  a = rng.rand((m, k), 31, dtype)
  b = rng.rand((k, n), 32, dtype)
  got = expr.dot(expr.from_numpy(a), expr.from_numpy(b)).glom()
  assert got.dtype == dtype
  cpu = O.dot_tiles(a, b, W)
  exact = a.astype(np.float64) @ b.astype(np.float64)
  check_fp(got, cpu, exact, rtol)


@pytest.mark.parametrize('dtype,rtol', [(np.float32, 1e-5), (np.float64, 1e-12)])
def test_dot_cfg4_full_size(ex, dtype, rtol):
  """configs[3] at its BASELINE size, 32768^2 (K = 32768 accumulation depth),
  through the same expr.dot the bench times.  Size-independent properties
  checked in fp64 on the device: row sums of C equal A . (B 1) and column
  sums equal (1^T A) . B; plus spot elements against an fp64 host dot of
  the generator's own values, under the CPU-or-closer rule (rtol 1e-5 fp32,
  1e-12 fp64; reference dot.py:238-283)."""
  expr, setw = ex
  setw(1)
  S = 32768
  f64 = np.float64
  A = expr.rand(S, S, dtype=dtype, seed=31).force()
  B = expr.rand(S, S, dtype=dtype, seed=32).force()
  Ae, Be = expr.lazify(A), expr.lazify(B)
  C = expr.dot(Ae, Be).force()
  Ce = expr.lazify(C)
  # row sums: sum_j C[i, j] = A[i, :] . rowsum(B)
  b1 = expr.sum(expr.astype(Be, f64), axis=1).glom()
  want_rows = expr.dot(expr.astype(Ae, f64), b1).glom()
  got_rows = expr.sum(expr.astype(Ce, f64), axis=1).glom()
  a0 = expr.sum(expr.astype(Ae, f64), axis=0).glom()
  want_cols = expr.dot(expr.transpose(expr.astype(Be, f64)), a0).glom()
  got_cols = expr.sum(expr.astype(Ce, f64), axis=0).glom()
  for got, want in ((got_rows, want_rows), (got_cols, want_cols)):
    rel = np.abs(got - want) / np.abs(want)
    assert rel.max() <= rtol, 'max rel err %g' % rel.max()
  # spot elements vs the generator's values on the host
  rows = [0, 1, 4097, 16383, 20000, 32767]
  cols = [0, 5, 8191, 16384, 30001, 32767]
  k = np.arange(S, dtype=np.uint64)
  for r in rows:
    crow = Ce[r:r + 1, :].glom().reshape(S)
    arow = rng.uniform_values(np.uint64(r * S) + k, 31, 0.0, 1.0, dtype)
    for c in cols:
      bcol = rng.uniform_values(k * np.uint64(S) + np.uint64(c), 32, 0.0, 1.0, dtype)
      cpu = np.dot(arow, bcol)
      exact = np.dot(arow.astype(f64), bcol.astype(f64))
      check_fp(np.array([crow[c]]), np.array([cpu]), np.array([exact]), rtol)
  # the margin (round-5 review): max |gpu - fp64| / |fp64| over EVERY element
  # of C (2^30 of them: the rows and columns with the largest |A| / |B| sums
  # included), against fp64 products of the same device values -- torch fp64
  # GEMMs on the device in 2048-row blocks, a checker only.  Asserted at 60 %
  # of the tolerance (40 % of the budget in reserve); printed for DESIGN 3.2.
  import torch
  (ta,), (tb,), (tc,) = ([t.data for t in X.local.values()] for X in (A, B, C))
  b64 = tb.to(torch.float64)
  margin, where = 0.0, None
  edges = torch.tensor([1e-7, 3e-7, 1e-6, 2e-6, 3e-6, 4e-6, 6e-6], dtype=torch.float64, device=tc.device) * (rtol / 1e-5)
  hist = torch.zeros(len(edges) + 1, dtype=torch.int64, device=tc.device)
  for r0 in range(0, S, 2048):
    want = ta[r0:r0 + 2048].to(torch.float64) @ b64
    rel = (tc[r0:r0 + 2048].to(torch.float64) - want).abs_().div_(want.abs())
    m = rel.max().item()
    if m > margin:
      i = int(rel.argmax())
      margin, where = m, (r0 + i // S, i % S)
    hist += torch.bincount(torch.bucketize(rel.flatten(), edges), minlength=len(edges) + 1)
    del want, rel
  del b64
  print('cfg4 %s margin: max rel err %.4g at C%s over all %d elements, tolerance %g; elements per '
        'rel-err bin (upper edges %s, last open): %s' % (np.dtype(dtype).name, margin, where, S * S, rtol,
                                                        ['%.3g' % e for e in edges.tolist()], hist.tolist()))
  assert margin <= 0.6 * rtol, 'cfg4 %s max rel err %.4g > 0.6 x %g' % (np.dtype(dtype).name, margin, rtol)
  # one FULL row and one FULL column of C against host dots over the whole of
  # B / A (the device values, bit-exact to the generator by
  # test_rand_bit_exact), streamed in 4096-row blocks: the dtype's own dot
  # (the CPU reference) and the fp64-exact one, same rule
  r, c = 20000, 30001
  crow = Ce[r:r + 1, :].glom().reshape(S)
  ccol = Ce[:, c:c + 1].glom().reshape(S)
  arow = Ae[r:r + 1, :].glom().reshape(S)
  bcol = Be[:, c:c + 1].glom().reshape(S)
  row_cpu = np.zeros(S, dtype)
  row_ex = np.zeros(S, f64)
  col_cpu = np.zeros(S, dtype)
  col_ex = np.zeros(S, f64)
  for k0 in range(0, S, 4096):
    bblk = Be[k0:k0 + 4096, :].glom()
    row_cpu += arow[k0:k0 + 4096] @ bblk
    row_ex += arow[k0:k0 + 4096].astype(f64) @ bblk.astype(f64)
    ablk = Ae[k0:k0 + 4096, :].glom()
    col_cpu[k0:k0 + 4096] = ablk @ bcol
    col_ex[k0:k0 + 4096] = ablk.astype(f64) @ bcol.astype(f64)
    del bblk, ablk
  check_fp(crow, row_cpu, row_ex, rtol)
  check_fp(ccol, col_cpu, col_ex, rtol)
  del A, B, C, Ae, Be, Ce


def test_gemm_layout_asymmetric(ex):
  """A = I with an asymmetric B catches a transposed C write."""
  expr, setw = ex
  setw(1)
  for dt in (np.float32, np.float64):
    a = np.eye(128, dtype=dt)
    b = np.arange(128 * 128, dtype=dt).reshape(128, 128) % 97
    np.testing.assert_array_equal(expr.dot(expr.from_numpy(a), expr.from_numpy(b)).glom(), b)


# ------------------------------------------------ fills (bit-exact generator)
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
@pytest.mark.parametrize('W', [1, 3])
def test_rand_bit_exact(ex, dtype, W):
  expr, setw = ex
  setw(W)
  got = expr.rand(97, 53, dtype=dtype, seed=7).glom()
  np.testing.assert_array_equal(got, rng.rand((97, 53), 7, dtype))
  got = expr.rand(64, 33, dtype=dtype, seed=8, low=-1.0, high=1.0).glom()
  np.testing.assert_array_equal(got, rng.rand((64, 33), 8, dtype, -1.0, 1.0))


# ------------------------------------------------ cfg2 class: fused map+reduce
def _cfg2_inputs(shape):
  x = rng.rand(shape, 11, np.float32)
  y = rng.rand(shape, 12, np.float32)
  z = rng.rand(shape, 13, np.float32, -1.0, 1.0)
  return x, y, z


@pytest.mark.parametrize('shape', [(96, 80), (257, 131), (1024, 3000)])
@pytest.mark.parametrize('W', [1, 2, 3, 8])
def test_fused_map_reduce_cfg2(ex, shape, W):
  expr, setw = ex
  setw(W)
  nx, ny, nz = _cfg2_inputs(shape)
  x = expr.rand(*shape, dtype=np.float32, seed=11)
  y = expr.rand(*shape, dtype=np.float32, seed=12)
  z = expr.rand(*shape, dtype=np.float32, seed=13, low=-1.0, high=1.0)
  mapped = O.map_tiles(lambda a, b, c: a * b + np.exp(c), [nx, ny, nz], W)
  # materialised map: elementwise, within 1e-5 relative of the CPU result
  m = (x * y + expr.exp(z)).optimized().glom()
  np.testing.assert_allclose(m, mapped, rtol=1e-6)
  exact_src = mapped.astype(np.float64)
  for axis in [None, 0, 1]:
    got = expr.sum(x * y + expr.exp(z), axis=axis).optimized().glom()
    cpu = O.sum_tiles(mapped, axis, W)
    check_fp(got, cpu, exact_src.sum(axis), 1e-5)
    for red, oref in [(expr.min, O.min_tiles), (expr.max, O.max_tiles)]:
      got = red(x * y + expr.exp(z), axis=axis).optimized().glom()
      # a min / max only selects an element: bit-exact against the reference's
      # tile-wise reduction of the GPU's own materialised map (whatever ulps
      # OCML's exp differs from NumPy's by), and within 1e-6 of the host map's
      np.testing.assert_array_equal(got, oref(m, axis, W))
      np.testing.assert_allclose(got, oref(mapped, axis, W), rtol=1e-6)
    for kind in ['argmin', 'argmax']:
      got = getattr(expr, kind)(x * y + expr.exp(z), axis=axis).optimized().glom()
      # bit-exact against the reference's three-pass argmin over the GPU's own
      # materialised map (the fused kernel evaluates the same generated tree,
      # so this holds whatever ulps OCML's exp differs from NumPy's by)
      np.testing.assert_array_equal(got, O.arg_tiles(m, axis, W, kind))
      if (m == mapped).all():
        np.testing.assert_array_equal(got, O.arg_tiles(mapped, axis, W, kind))


def test_arg_axis_none_block_tiles(ex):
  """The documented axis=None divergence: (2, 100)
  at W = 3 is tiled in blocks of (1, 66) (good_tile_shape fills the last
  axis first), so the reference's _arg_mapper ravels a tile's local index
  with the TILE shape (builtins.py:618-624, restated by the oracle) and
  returns a position that is not NumPy's flat index; this build returns
  NumPy's.  Both answers are stated here."""
  expr, setw = ex
  setw(3)
  a = np.full((2, 100), 5.0)
  a[1, 70] = -3.0   # min in the (1, 66:100) block
  a[0, 10] = 9.0    # max in the first block
  from spartan_amd.array import distarray
  tiles = sorted((ex_.ul, ex_.lr) for ex_ in distarray.from_numpy(a).tiles)
  assert tiles[0] == ((0, 0), (1, 66)), tiles
  x = expr.from_numpy(a)
  got_min = int(expr.argmin(x).glom())
  got_max = int(expr.argmax(x).glom())
  assert got_min == int(np.argmin(a)) == 170
  assert got_max == int(np.argmax(a)) == 10
  # the reference's answer: ravelled_pos((1, 66) + (0, 4), tile shape (1, 34)) = 104
  ref_min = int(O.arg_tiles(a, None, 3, 'argmin'))
  ref_max = int(O.arg_tiles(a, None, 3, 'argmax'))
  assert ref_min == 104 and ref_min != got_min
  assert ref_max == 10 == got_max  # first block: ul = 0, both agree


@pytest.mark.parametrize('W', [1, 3, 4])
def test_argmin_ties_cross_tiles(ex, W):
  expr, setw = ex
  setw(W)
  a = np.zeros((12, 10), dtype=np.float64)
  a[3, 4] = a[7, 4] = a[11, 9] = -5.0  # ties in different row strips
  a[5, :] = -1.0
  x = expr.from_numpy(a)
  for axis in [None, 0, 1]:
    np.testing.assert_array_equal(x.argmin(axis).glom(), a.argmin(axis))
    np.testing.assert_array_equal(x.argmin(axis).glom(), O.arg_tiles(a, axis, W))
    np.testing.assert_array_equal((-x).argmax(axis).glom(), (-a).argmax(axis))


def _big_int_arrays():
  """int64 values around 2^60 (float64 cannot tell v from v+1 there): the
  winner sits in a later row block / partial than values 1 away from it."""
  base = 2 ** 60
  out = []
  a = np.full((12, 10), base, dtype=np.int64)
  a[11, 7] = base + 1
  a[10, 2] = base - 1
  out.append(a)
  # several partials per output (rows / cols kernels split R across blocks)
  b = np.full((6, 200000), base, dtype=np.int64)
  b[:, 150001] = base + 3
  b[:, 170003] = base - 3
  b[4, 199999] = base + 4
  out.append(b)
  c = np.full((300000, 3), base, dtype=np.int64)
  c[250000, :] = base + 1
  c[299999, 1] = base - 1
  out.append(c)
  d = np.full((2048, 2048), base, dtype=np.int64)
  d[2000, 2040] = base + 1
  d[1999, 5] = base - 1
  out.append(d)
  return out


@pytest.mark.parametrize('W', [1, 3])
def test_int64_arg_above_2p53(ex, W):
  """argmin / argmax over int64 near 2^60 are bit-exact across blocks, tiles
  and partial combines (the combine compares int64, not float64)."""
  expr, setw = ex
  setw(W)
  for a in _big_int_arrays():
    x = expr.from_numpy(a)
    for axis in [None, 0, 1]:
      for kind in ['argmin', 'argmax']:
        got = getattr(x, kind)(axis).glom()
        np.testing.assert_array_equal(got, getattr(a, kind)(axis), err_msg='%s %s %s' % (a.shape, axis, kind))
        np.testing.assert_array_equal(got, O.arg_tiles(a, axis, W, kind))
      np.testing.assert_array_equal(expr.max(x, axis).glom(), a.max(axis))
      np.testing.assert_array_equal(expr.min(x, axis).glom(), a.min(axis))


def test_empty_and_ragged(ex):
  expr, setw = ex
  setw(3)
  for shape in [(1,), (2,), (5, 1), (1, 7), (3, 3, 1), (7, 13)]:
    n = np.arange(int(np.prod(shape)), dtype=np.float64).reshape(shape) - 3.5
    x = expr.from_numpy(n)
    for axis in [None] + list(range(len(shape))):
      np.testing.assert_array_equal(x.sum(axis).glom(), n.sum(axis))
      np.testing.assert_array_equal(x.max(axis).glom() if hasattr(x, 'max') else expr.max(x, axis).glom(),
                                    n.max(axis))
      np.testing.assert_array_equal(x.argmin(axis).glom(), n.argmin(axis))


def test_int32_and_bool_semantics(ex):
  expr, setw = ex
  setw(3)
  n = (np.arange(60, dtype=np.int32).reshape(6, 10) * 1000003)
  x = expr.from_numpy(n)
  for axis in [None, 0, 1]:
    got = x.sum(axis).glom()
    assert got.dtype == np.int32
    np.testing.assert_array_equal(got, O.sum_tiles(n, axis, 3))
  b = expr.from_numpy(n % 3 == 0)
  np.testing.assert_array_equal(expr.count_nonzero(b).glom(), np.count_nonzero(n % 3 == 0))
  m = expr.mean(x, 0).glom()
  np.testing.assert_array_equal(m, n.sum(0) // 6)


@pytest.mark.parametrize('dt', [np.int32, np.int64])
def test_small_int_min_max_arg(ex, dt):
  """min / max / argmin / argmax keep the value type: the identity is that
  type's extreme (all-positive and all-negative inputs, ties at the extremes,
  each of the rows / rowsp / cols skeletons)."""
  expr, setw = ex
  setw(3)
  ii = np.iinfo(dt)
  rng = np.random.default_rng(7)
  for shape in [(6, 10), (7, 3000), (3000, 5)]:
    for lo, hi in [(1, 100), (ii.min, ii.min // 2 if ii.min < 0 else 1), (ii.max - 3, ii.max)]:
      n = rng.integers(lo, int(hi) + 1, size=shape, dtype=np.int64).astype(dt)
      x = expr.from_numpy(n)
      for axis in [None, 0, 1]:
        for fe, fn in [(expr.min, np.min), (expr.max, np.max), (expr.argmin, np.argmin), (expr.argmax, np.argmax)]:
          got = fe(x, axis=axis).glom()
          np.testing.assert_array_equal(got, fn(n, axis=axis), err_msg='%s %s %s %s' % (dt, shape, axis, fn.__name__))


def test_full_size_checksums(ex):
  """cfg2 at its BASELINE size (2^30 fp32): size-independent properties --
  the axis-0, axis-1 and full sums agree (checksum of checksums) and the
  reductions equal the reduction of the materialised map."""
  expr, setw = ex
  setw(1)
  shape = (32768, 32768)
  x = expr.rand(*shape, dtype=np.float32, seed=11).force()
  y = expr.rand(*shape, dtype=np.float32, seed=12).force()
  z = expr.rand(*shape, dtype=np.float32, seed=13, low=-1.0, high=1.0).force()
  xs, ys, zs = expr.lazify(x), expr.lazify(y), expr.lazify(z)
  s0 = expr.sum(xs * ys + expr.exp(zs), axis=0).optimized().glom().astype(np.float64)
  s1 = expr.sum(xs * ys + expr.exp(zs), axis=1).optimized().glom().astype(np.float64)
  s = float(expr.sum(xs * ys + expr.exp(zs)).optimized().glom())
  assert s0.shape == (32768,) and s1.shape == (32768,)
  assert abs(s0.sum() - s1.sum()) <= 1e-5 * abs(s1.sum())
  assert abs(s - s1.sum()) <= 1e-5 * abs(s1.sum())
  # E[x*y + exp(z)] = 1/4 + (e - 1/e)/2
  mean = s / (32768.0 * 32768.0)
  assert abs(mean - (0.25 + (np.e - 1 / np.e) / 2)) < 1e-3
  # spot rows against the oracle restatement
  for r in (0, 12345, 32767):
    g = np.arange(r * 32768, (r + 1) * 32768, dtype=np.uint64)
    row = (rng.uniform_values(g, 11, 0.0, 1.0, np.float32) * rng.uniform_values(g, 12, 0.0, 1.0, np.float32)
           + np.exp(rng.uniform_values(g, 13, -1.0, 1.0, np.float32)))
    check_fp(s1[r:r + 1].astype(np.float32), np.array([row.sum()], np.float32),
             np.array([row.astype(np.float64).sum()]), 1e-5)


def test_lreg_cfg5_full_size(ex):
  """cfg5 at its BASELINE size (X 1e8 x 64 fp32): the fused one-pass
  gradient equals an fp64 restatement computed chunk by chunk on the device
  (X^T (X w - y) with torch fp64 matmuls) within the fp32 rule."""
  import torch
  expr, setw = ex
  setw(1)
  n, d = 100_000_000, 64
  X = expr.rand(n, d, dtype=np.float32, seed=41).force()
  Y = expr.rand(n, 1, dtype=np.float32, seed=42).force()
  w = (np.random.default_rng(43).random((d, 1)) - 0.5).astype(np.float32)
  got = expr.sum(expr.lazify(X) * (expr.dot(expr.lazify(X), w) - expr.lazify(Y)), axis=0).optimized().glom()
  xt = next(iter(X.local.values())).data
  yt = next(iter(Y.local.values())).data
  wd = torch.as_tensor(w, dtype=torch.float64, device=xt.device)
  acc = torch.zeros((d,), dtype=torch.float64, device=xt.device)
  for r0 in range(0, n, 10_000_000):
    xc = xt[r0:r0 + 10_000_000].to(torch.float64)
    acc += (xc * (xc @ wd - yt[r0:r0 + 10_000_000].to(torch.float64))).sum(0)
  exact = acc.cpu().numpy()
  # per column: within 1e-5 of the exact column (the strict fp32 rule; these
  # columns are well conditioned, sum|terms| / |sum| ~ 1) and, beyond the
  # rounding of the result to fp32 (half an ulp), within 2e-8 of the column's
  # own sum_i |x_ij| |r_i| (bench.check_lreg's condition)
  acn = torch.zeros((d,), dtype=torch.float64, device=xt.device)
  for r0 in range(0, n, 10_000_000):
    xc = xt[r0:r0 + 10_000_000].to(torch.float64)
    acn += torch.mv(xc.abs().t(), (xc @ wd - yt[r0:r0 + 10_000_000].to(torch.float64)).abs().reshape(-1))
  cond = acn.cpu().numpy()
  err = np.abs(np.asarray(got, np.float64).reshape(-1) - exact.reshape(-1))
  half_ulp = 0.5 * np.spacing(np.abs(exact.reshape(-1)).astype(np.float32)).astype(np.float64)
  excess = np.maximum(err - half_ulp, 0.0)
  print('lreg cfg5 full size: max rel err %.3g, max err / ulp %.3g, max excess / sum|terms| %.3g'
        % ((err / np.abs(exact)).max(), (err / (2 * half_ulp)).max(), (excess / cond).max()))
  assert np.all(err <= 1e-5 * np.abs(exact))
  assert np.all(excess <= 2e-8 * cond)


def test_kmeans_cfg3_full_size(ex):
  """cfg3 at its BASELINE size (1e8 x 128 fp32, k = 256, second-iteration
  centres): the certified assignment equals the all-exact kernel on a 2M-row
  prefix and on 2M rows at the end, and on ALL 1e8 rows the default path (fp16
  screen + bf16x3 list pass) equals the bf16x3 pass over every row (two
  independently certified filters); the fp64 centroid sums and counts equal a
  chunked torch index_add restatement (counts exact, sums within 1e-12)."""
  import torch
  from spartan_amd import backend
  expr, setw = ex
  setw(1)
  be = backend.get()
  N, D, K = 100_000_000, 128, 256
  dev = torch.device('cuda:0')
  pts = torch.empty((N, D), dtype=torch.float32, device=dev)
  be.fill(pts, backend.FILL_UNIFORM, 0.0, 1.0, 21, (0, 0), (N, D))
  lab = torch.empty((N,), dtype=torch.int64, device=dev)
  sums = torch.empty((K, D), dtype=torch.float64, device=dev)
  cnt = torch.empty((K,), dtype=torch.int64, device=dev)
  be.kmeans_assign(pts, pts[:K].to(torch.float64).contiguous(), lab)
  be.kmeans_accumulate(pts, lab, sums, cnt)
  cen = (sums / cnt.clamp(min=1).to(torch.float64).reshape(K, 1)).contiguous()
  be.kmeans_assign(pts, cen, lab)
  for a, b in ((0, 2_000_000), (N - 2_000_000, N)):
    ref = torch.empty((b - a,), dtype=torch.int64, device=dev)
    be.kmeans_assign(pts[a:b], cen, ref, exact_only=True)
    assert torch.equal(lab[a:b], ref)
  # the fused step (B-stationary screen + accumulation, one pass) against
  # the A-stationary screen's labels on every row: two certified screens
  lab_st = torch.empty_like(lab)
  s_st = torch.empty_like(sums)
  c_st = torch.empty_like(cnt)
  be.kmeans_step(pts, cen, lab_st, s_st, c_st)
  assert torch.equal(lab_st, lab)
  del lab_st
  be.kmeans_accumulate(pts, lab, sums, cnt)
  s2 = torch.zeros((K, D), dtype=torch.float64, device=dev)
  c2 = torch.zeros((K,), dtype=torch.int64, device=dev)
  for r0 in range(0, N, 10_000_000):
    li = lab[r0:r0 + 10_000_000]
    s2.index_add_(0, li, pts[r0:r0 + 10_000_000].to(torch.float64))
    c2 += torch.bincount(li, minlength=K)
  assert torch.equal(cnt, c2) and int(cnt.sum()) == N
  torch.testing.assert_close(sums, s2, rtol=1e-12, atol=1e-9)
  assert torch.equal(c_st, c2)
  torch.testing.assert_close(s_st, s2, rtol=1e-6, atol=0)   # fp32 chains of <= 255 tiles per block


# ------------------------------------------------------ cfg5: lreg gradient
@pytest.mark.parametrize('W', [1, 3])
def test_lreg_cfg5_small(ex, W):
  from oracle import workloads as OW
  from spartan_amd import workloads
  expr, setw = ex
  setw(W)
  n, d = 10000, 64
  X = rng.rand((n, d), 41, np.float32)
  Yv = rng.rand((n, 1), 42, np.float32)
  w = rng.rand((d, 1), 43, np.float32)
  x = expr.rand(n, d, dtype=np.float32, seed=41)
  y = expr.rand(n, 1, dtype=np.float32, seed=42)
  alpha = 1e-6
  got = workloads.linear_regression_update(x, y, w, alpha)
  want = OW.linear_regression_update(X, Yv, w, alpha, W)
  # the update differs from the CPU one by alpha * (gradient difference): bound it
  # by the gradient tolerance (1e-5 relative) -- the gradient is checked below
  gmax = np.abs((X.astype(np.float64) * (X.astype(np.float64) @ w - Yv)).sum(0)).max()
  np.testing.assert_allclose(got, want, rtol=0, atol=alpha * 1e-5 * gmax + 1e-7)
  # gradient itself (not damped by alpha): vs fp64 exact and the CPU path
  yp = expr.dot(x, w).glom()
  np.testing.assert_allclose(yp, X @ w, rtol=2e-6)
  g = expr.sum(x * (expr.dot(x, w) - y), axis=0).optimized().glom()
  exact = (X.astype(np.float64) * (X.astype(np.float64) @ w.astype(np.float64) - Yv)).sum(0)
  cpu = (X * (X @ w - Yv)).sum(0)
  check_fp(g, cpu, exact, 1e-5)


@pytest.mark.parametrize('W', [1, 3])
def test_replayed_plans_follow_new_values(ex, W):
  """An iterative driver's DAG is replayed (plan cache), its LocalExpr tree
  lowered once (engine bind memo) and its reduction relaunched from a
  recorded launch plan (backend.reduce): every iteration must still see its
  own host vector, scalars and arrays -- checked against NumPy per step,
  with a shape change in between (a different plan, then back)."""
  from spartan_amd import backend
  expr, setw = ex
  setw(W)
  n, d = 3000, 64
  X = rng.rand((n, d), 41, np.float32)
  Yv = rng.rand((n, 1), 42, np.float32)
  x = expr.lazify(expr.rand(n, d, dtype=np.float32, seed=41).force())
  y = expr.lazify(expr.rand(n, 1, dtype=np.float32, seed=42).force())
  be = backend.get()
  g = np.random.default_rng(5)
  for it in range(6):
    w = g.random((d, 1)).astype(np.float32) - 0.5
    a = float(g.random()) * 4 - 2
    got = expr.sum(x * (expr.dot(x, w) - y), axis=0).optimized().glom()
    exact = (X.astype(np.float64) * (X.astype(np.float64) @ w.astype(np.float64) - Yv)).sum(0)
    check_fp(got, (X * (X @ w - Yv)).sum(0), exact, 1e-5)
    got2 = expr.sum(x * a + 1.5, axis=1).optimized().glom()
    exact2 = (X.astype(np.float64) * a + 1.5).sum(1)
    check_fp(got2, (X * np.float32(a) + np.float32(1.5)).sum(1), exact2, 1e-5)
    if it == 2:  # another shape, then the first one again
      xs = expr.rand(n // 2, d, dtype=np.float32, seed=41)
      got3 = expr.sum(xs * (expr.dot(xs, w) - 1.0), axis=0).optimized().glom()
      Xs = X[:n // 2]  # counter-based generator: same flat indices
      e3 = (Xs.astype(np.float64) * (Xs.astype(np.float64) @ w.astype(np.float64) - 1.0)).sum(0)
      check_fp(got3, (Xs * (Xs @ w - np.float32(1.0))).sum(0), e3, 1e-5)
  assert be._reduce_plans  # the replay path was taken


def _backend_reduce(be, t, op, axis):
  """backend.reduce of the fp32 device tensor ``t`` itself (no expr layer)
  as a NumPy array; arg ops: the indices."""
  from spartan_amd import codegen
  shape = tuple(t.shape)
  oshape = () if axis is None else shape[:axis] + shape[axis + 1:]
  arg = op in ('argmin', 'argmax')
  r = be.reduce(codegen.In(0, np.float32), op, {0: t}, shape, axis, oshape, np.int64 if arg else np.float32,
                {'offset': 0} if arg else None)
  return (r[1] if arg else r).cpu().numpy()


@pytest.mark.parametrize('shape,axis,op,kind,grid', [((3, 5000), 1, 'sum', 'rows', 3 * 2),
                                                     ((5000, 8), 0, 'sum', 'cols', 10),
                                                     ((5000, 8), 0, 'argmin', 'cols', 10)])
def test_reduce_first_call_and_replay_identical(ex, shape, axis, op, kind, grid):
  """One executor launches a planned reduction on its first call and on every
  replay: both results are bit-identical and match NumPy, and the replay adds
  neither a launch plan nor a kernel.  grid = segments x P partials each
  (P = 2 / 10: the finalize pass runs)."""
  import torch
  from spartan_amd import backend
  ex[1](1)
  be = backend.get()
  X = rng.rand(shape, 77, np.float32) - np.float32(0.5)
  t = torch.as_tensor(X).cuda()
  be._reduce_plans.clear()
  be.launch_log = []
  try:
    first = _backend_reduce(be, t, op, axis)
    counts = (len(be._reduce_plans), len(be._sig_fns), len(be._fns))
    again = _backend_reduce(be, t, op, axis)
    assert be.launch_log == [grid, grid]
  finally:
    be.launch_log = None
  assert counts[0] == 1 and (len(be._reduce_plans), len(be._sig_fns), len(be._fns)) == counts
  assert [k for k in be._sig_fns if k[0] == 'reduce' and k[4:6] == (kind, op)]
  np.testing.assert_array_equal(first, again)
  if op == 'argmin':
    np.testing.assert_array_equal(first, X.argmin(axis))
  else:
    check_fp(first, X.sum(axis), X.astype(np.float64).sum(axis), 1e-5)


def test_reduce_strided_view_twice(ex):
  """A strided view whose dims do not collapse to (O, R, I) is copied dense on
  every call: the second call of the same view must not relaunch the copy's
  plan on the view's own pointer."""
  import torch
  from spartan_amd import backend
  ex[1](1)
  be = backend.get()
  X = rng.rand((6, 10, 8), 78, np.float32)
  v = torch.as_tensor(X).cuda()[:, ::2, ::2]
  for axis in (None, 0):
    first, again = _backend_reduce(be, v, 'sum', axis), _backend_reduce(be, v, 'sum', axis)
    np.testing.assert_array_equal(first, again)
    check_fp(first, X[:, ::2, ::2].sum(axis), X[:, ::2, ::2].astype(np.float64).sum(axis), 1e-5)


def _rowdot_exact(X, w, Yv):
  """(sum(x * (x w - y), axis=0), x w - y) as float64 arrays, computed in
  float64 for fp32 inputs and in extended precision (np.longdouble, 64-bit
  significand on x86) for fp64 inputs -- an fp64 'exact' value carries
  errors as large as the fp64 kernel's own."""
  hp = np.float64 if X.dtype == np.float32 else np.longdouble
  Xh = X.astype(hp)
  r = Xh @ w.astype(hp) - Yv.astype(hp)
  return (Xh * r).sum(0).astype(np.float64), r.astype(np.float64)


@pytest.mark.parametrize('K,dt', [(64, np.float32), (48, np.float32), (5, np.float32), (2, np.float32),
                                  (64, np.float64), (33, np.float64)])
@pytest.mark.parametrize('W', [1, 3])
def test_dot_reduce_fusion(ex, K, dt, W):
  """DotReduceFusion: sum(x * (dot(x, w) - y), axis=0) runs as ONE generated
  column-reduce kernel with the row dot inside (DPP row sums); K not a power
  of two exercises the zero-filled lanes, K=5 fp32 / K=33 fp64 the unaligned
  scalar path.  Tolerances: as the CPU result (1e-5 fp32, 1e-12 fp64)."""
  from spartan_amd.expr.dot import DotExpr
  expr, setw = ex
  setw(W)
  n = 7001
  X = rng.rand((n, K), 41, dt) - dt(0.5)
  Yv = rng.rand((n, 1), 42, dt)
  w = rng.rand((K, 1), 43, dt) - dt(0.25)
  x, y = expr.from_numpy(X), expr.from_numpy(Yv)
  e = expr.sum(x * (expr.dot(x, w) - y), axis=0).optimized()
  assert not any(isinstance(c, DotExpr) for c in e.children)
  got = e.glom()
  exact, r64 = _rowdot_exact(X, w, Yv)
  yp = np.concatenate([X[ex[0][0]:ex[1][0]].dot(w) for ex, _ in O.compute_extents(X.shape, W)])
  cpu = O.sum_tiles(X * (yp - Yv), 0, W)
  # centred X and w: some columns cancel to ~1e-5 of their sum |terms| (the
  # condition-aware pass of check_fp, round 5)
  cond = (np.abs(X.astype(np.float64)) * np.abs(r64)).sum(0)
  rtol = 1e-5 if dt == np.float32 else 1e-12
  n_cond, ratio = check_fp(got, cpu, exact, rtol, cond)
  # round 6: the interleaved kernel's chunk sums fold into fp64 (Kahan for
  # fp64 inputs), so the escape should be (nearly) unused: report how many
  # elements needed it and bound the worst error against sum |terms| at a
  # fifth of the escape's own threshold
  print('dot_reduce_fusion K=%d %s W=%d: n_cond=%d of %d, max |gpu-exact|/sum|terms| = %.3g (bound %.3g)'
        % (K, np.dtype(dt).name, W, n_cond, K, ratio, 0.2 * 1e-2 * rtol))
  assert ratio <= 0.2 * 1e-2 * rtol
  assert n_cond <= 1


@pytest.mark.parametrize('dt', [np.float32, np.float64])
@pytest.mark.parametrize('interleave,bpc', [(True, 1), (True, 16), (False, 1), (False, 16)])
def test_rowdot_knobs(ex, monkeypatch, interleave, bpc, dt):
  """The row-dot kernel's layout knobs (backend.ROWDOT_INTERLEAVE /
  ROWDOT_BLOCKS_PER_CU change the generated kernel and its grid): sum and max
  of x * (dot(x, w) - y) over axis 0 for each setting, at a row count that is
  no multiple of U * 16 * P and large enough (1.1M rows) that one block per
  CU folds its fp64 middle sums into the total (>= 32 super-chunks per
  block).  Sums: check_fp, with the worst error against sum |terms| bounded at
  a fifth of the condition escape's threshold and the escape's use printed;
  max: within the row dot's rounding of the fp64 value."""
  from spartan_amd import backend
  from spartan_amd.expr.dot import DotExpr
  expr, setw = ex
  setw(1)
  monkeypatch.setattr(backend, 'ROWDOT_INTERLEAVE', interleave)
  monkeypatch.setattr(backend, 'ROWDOT_BLOCKS_PER_CU', bpc)
  n, K = 1_100_003, 64
  X = rng.rand((n, K), 41, dt) - dt(0.5)
  Yv = rng.rand((n, 1), 42, dt)
  w = rng.rand((K, 1), 43, dt) - dt(0.25)
  x, y = expr.from_numpy(X), expr.from_numpy(Yv)
  rtol = 1e-5 if dt == np.float32 else 1e-12
  e = expr.sum(x * (expr.dot(x, w) - y), axis=0).optimized()
  assert not any(isinstance(c, DotExpr) for c in e.children)
  got = e.glom()
  exact, r64 = _rowdot_exact(X, w, Yv)
  cpu = (X * (X @ w - Yv)).sum(0, dtype=dt)
  cond = (np.abs(X.astype(np.float64)) * np.abs(r64)).sum(0)
  n_cond, ratio = check_fp(got, cpu, exact, rtol, cond)
  print('rowdot knobs interleave=%s bpc=%d %s: n_cond=%d, max err/sum|terms| %.3g'
        % (interleave, bpc, np.dtype(dt).name, n_cond, ratio))
  assert ratio <= 0.2 * 1e-2 * rtol
  mx = expr.max(x * (expr.dot(x, w) - y), axis=0).optimized()
  assert not any(isinstance(c, DotExpr) for c in mx.children)
  gm = np.asarray(mx.glom(), np.float64)
  em = (X.astype(np.float64) * r64).max(0)
  # one row's value x * (rd - y): rd an fp32 / fp64 dot of K terms
  tol = 4 * K * np.finfo(dt).eps * (np.abs(X).max(0) * (np.abs(X) @ np.abs(w) + np.abs(Yv)).max())
  assert np.all(np.abs(gm - em) <= tol)


@pytest.mark.parametrize('W', [1, 3])
def test_sgd_device_w_matches_host(ex, W):
  """sgd_train with w resident on the GPU (DotReduceFusion over a device
  (K, 1) operand + a device update map) equals the reference's host form
  bit for bit, and the fused kernel runs (no DotExpr left)."""
  from spartan_amd import workloads
  from spartan_amd.expr.dot import DotExpr
  expr, setw = ex
  setw(W)
  n, K = 20011, 64
  X = rng.rand((n, K), 41, np.float32)
  Yv = rng.rand((n, 1), 42, np.float32)
  w = rng.rand((K, 1), 43, np.float32)
  x = expr.lazify(expr.from_numpy(X).force())
  y = expr.lazify(expr.from_numpy(Yv).force())
  Wd = expr.lazify(expr.from_numpy(w).force())
  e = expr.sum(x * (expr.dot(x, Wd) - y), axis=0).optimized()
  assert not any(isinstance(c, DotExpr) for c in e.children)
  np.testing.assert_array_equal(e.glom(), expr.sum(x * (expr.dot(x, w) - y), axis=0).optimized().glom())
  w_dev = workloads.sgd_train(x, y, w, 1e-6, 4)
  w_host = workloads.sgd_train(x, y, w, 1e-6, 4, device_w=False)
  np.testing.assert_array_equal(w_dev, w_host)


# ---------------------------------------------- short rows (packed kernel)
@pytest.mark.parametrize('R', [1, 3, 64, 77, 256, 1000, 4096, 5000])
def test_short_rows(ex, R):
  expr, setw = ex
  setw(2)
  n = 300
  a = rng.rand((n, R), 5, np.float64) - 0.5
  x = expr.from_numpy(a)
  np.testing.assert_allclose(x.sum(1).glom(), a.sum(1), rtol=1e-12, atol=1e-12)
  np.testing.assert_array_equal(x.argmin(1).glom(), a.argmin(1))
  np.testing.assert_array_equal(x.argmax(1).glom(), a.argmax(1))
  np.testing.assert_array_equal(expr.max(x, 1).glom(), a.max(1))
  f = a.astype(np.float32)
  xf = expr.from_numpy(f)
  np.testing.assert_array_equal(xf.argmin(1).glom(), f.argmin(1))
  np.testing.assert_allclose(expr.sum(xf * xf, axis=1).optimized().glom(), (f * f).sum(1), rtol=1e-5)


# ------------------------------------------------------------ cfg3: k-means
@pytest.mark.parametrize('D,K', [(16, 8), (128, 256), (3, 70), (130, 5)])
@pytest.mark.parametrize('W', [1, 3])
def test_kmeans_assign_bit_exact(ex, D, K, W):
  """Labels must equal argmin(scipy cdist) bit for bit, ties -> first index."""
  from oracle import workloads as OW
  from spartan_amd import workloads
  expr, setw = ex
  setw(W)
  n = 5000
  pts = rng.rand((n, D), 21, np.float32)
  centers = pts[:K].astype(np.float64).copy()
  if K >= 4:
    centers[K - 1] = centers[1]          # exact duplicate centre: ties -> lower index
    pts[10] = ((centers[2] + centers[3]) / 2).astype(np.float32)  # near-equidistant point
  c, labels = workloads.kmeans_fit(expr.from_numpy(pts), K, 1, centers=centers)
  want = OW.kmeans_assign(pts, centers)
  np.testing.assert_array_equal(labels.glom(), want)
  c2, _ = OW.kmeans_fit(pts, K, 1, W, centers=centers)
  exact = np.zeros_like(c2)
  cnt = np.bincount(want, minlength=K)
  for i in range(K):
    exact[i] = pts[want == i].astype(np.float64).sum(0) / max(cnt[i], 1)
  nz = cnt > 0
  check_fp(c[nz], c2[nz], exact[nz], 1e-5)


def test_kmeans_fit_iterations(ex):
  from oracle import workloads as OW
  from spartan_amd import workloads
  expr, setw = ex
  setw(2)
  pts = rng.rand((20000, 32), 22, np.float32)
  c, labels = workloads.kmeans_fit(expr.from_numpy(pts), 16, 4)
  c2, l2 = OW.kmeans_fit(pts, 16, 4, 2)
  np.testing.assert_allclose(c, c2, rtol=1e-4)
  assert (labels.glom() == l2).mean() > 0.999


@pytest.mark.parametrize('case', ['plain', 'empty', 'screen'])
def test_kmeans_fit_speculation_identical(ex, case, monkeypatch):
  """workloads.kmeans_fit queues iteration i + 1 with device-divided centres
  before the host has read iteration i's counts: the centres, labels, sums
  and counts must be bit-identical to the sequential loop
  (SPARTAN_KMEANS_SPECULATE=0).  'empty': a centre far from every point (an
  empty cluster: the host reseeds it, the speculative step is re-run);
  'screen': the certified screen's domain (D = 128, K = 256)."""
  from spartan_amd import workloads
  expr, setw = ex
  setw(1)
  D, K, n = (128, 256, 60000) if case == 'screen' else (32, 16, 20000)
  pts = rng.rand((n, D), 23, np.float32)
  c0 = pts[:K].astype(np.float64).copy()
  if case == 'empty':
    c0[3] = 1e3
  runs = []
  for spec in ('0', '1'):
    monkeypatch.setenv('SPARTAN_KMEANS_SPECULATE', spec)
    info = {}
    c, lab = workloads.kmeans_fit(expr.from_numpy(pts), K, 3, centers=c0, info=info)
    runs.append((c, lab.glom(), info))
  (ca, la, ia), (cb, lb, ib) = runs
  assert np.array_equal(ca.view(np.int64), cb.view(np.int64))
  np.testing.assert_array_equal(la, lb)
  assert np.array_equal(ia['sums'].view(np.int64), ib['sums'].view(np.int64))
  np.testing.assert_array_equal(ia['counts'], ib['counts'])
  assert ia['speculated'] == 0 and ia['respun'] == 0
  assert ib['speculated'] + ib['respun'] == 2
  if case == 'empty':
    assert ib['respun'] >= 1
  else:
    assert ib['speculated'] == 2   # the device quotients matched the host's bit for bit


@pytest.mark.parametrize('case', ['plain', 'empty', 'd64'])
def test_kmeans_api_speculation_identical(ex, case, monkeypatch):
  """examples.kmeans.KMeans.fit (the reference's loop through outer / argmin
  / map2): the centre join queues the next fused step behind a pinned copy of
  the sums the host is about to read; the next assignment adopts it only for
  bit-identical centres.  Centres and labels must equal the run with
  SPARTAN_KMEANS_SPECULATE=0; 'plain' / 'd64' adopt every queued step,
  'empty' (a centre no point is nearest to: the host reseeds it) drops the
  one queued for the reseeded centres.  The fit leaves no host shadow or
  upload alias registered and keeps neither X nor the labels alive."""
  import gc
  import weakref
  from spartan_amd.array import transfer
  from spartan_amd.examples import kmeans as KM
  from spartan_amd.expr import plan_cache
  from spartan_amd.expr.base import eval_cache
  expr, setw = ex
  setw(1)
  D, K, n = (64, 32, 30000) if case == 'd64' else (128, 64, 40000)
  pts = rng.rand((n, D), 24, np.float32)
  c0 = pts[:K].astype(np.float64).copy()
  if case == 'empty':
    c0[5] = 1e3
  X = expr.from_numpy(pts).force()
  runs = []
  for spec in ('0', '1'):
    monkeypatch.setenv('SPARTAN_KMEANS_SPECULATE', spec)
    before = dict(KM.SPEC_STATS)
    c, lab = KM.KMeans(K, 3).fit(X, c0)
    stats = {k: KM.SPEC_STATS[k] - before[k] for k in before}
    runs.append((c, lab.glom(), stats))
  # nothing the speculating fit registered is left for a later download / upload to take
  assert not transfer._SHADOWS and not transfer._ALIAS
  (ca, la, sa), (cb, lb, sb) = runs
  assert np.array_equal(ca.view(np.int64), cb.view(np.int64))
  np.testing.assert_array_equal(la, lb)
  assert sa == {'queued': 0, 'adopted': 0, 'dropped': 0}
  assert sb['queued'] == 2, sb
  if case == 'empty':
    assert sb['dropped'] >= 1 and sb['adopted'] + sb['dropped'] == 2, sb
  else:
    assert sb['adopted'] == 2, sb
  # ... and the fit keeps neither X nor its labels alive
  wx, wl = weakref.ref(X), weakref.ref(lab.force())
  del X, lab
  eval_cache.clear()
  plan_cache.clear()
  gc.collect()
  assert wx() is None and wl() is None


@pytest.mark.parametrize('dt', [np.float32, np.float64])
@pytest.mark.parametrize('N,D,K', [(1, 3, 1), (1000, 16, 8), (70001, 128, 256), (9000, 130, 300),
                                   (5000, 300, 1100), (4097, 33, 7), (0, 8, 4)])
def test_kmeans_accumulate_direct(ex, dt, N, D, K):
  """Per-centre sums / counts against an fp64 NumPy sum (the reference sums in
  fp32 -- k_means_.py:67-89 -- fp64 is tighter); labels outside [0, K) are
  skipped; zero_first=False adds; the result is deterministic (no float
  atomics: repeated runs are bit-identical)."""
  import torch
  from spartan_amd import backend
  be = backend.get()
  g = np.random.default_rng(N + D + K)
  pts = g.standard_normal((N, D)).astype(dt)
  lab = g.integers(-1, K + 1, size=N).astype(np.int64)   # includes -1 and K: skipped
  P = torch.as_tensor(pts).cuda()
  L = torch.as_tensor(lab).cuda()
  sums = torch.full((K, D), 7.0, dtype=torch.float64, device='cuda')
  cnts = torch.full((K,), 3, dtype=torch.int64, device='cuda')
  be.kmeans_accumulate(P, L, sums, cnts, zero_first=True)
  s1, c1 = sums.cpu().numpy().copy(), cnts.cpu().numpy().copy()
  want_s = np.zeros((K, D))
  ok = (lab >= 0) & (lab < K)
  np.add.at(want_s, lab[ok], pts[ok].astype(np.float64))
  want_c = np.bincount(lab[ok], minlength=K)
  np.testing.assert_array_equal(c1, want_c)
  scale = np.sqrt(np.maximum(want_c, 1))[:, None] * np.abs(pts).max(initial=1.0)
  assert np.all(np.abs(s1 - want_s) <= 1e-13 * scale * max(1, N) ** 0.5 + 1e-300)
  be.kmeans_accumulate(P, L, sums, cnts, zero_first=True)
  np.testing.assert_array_equal(sums.cpu().numpy(), s1)        # deterministic
  be.kmeans_accumulate(P, L, sums, cnts, zero_first=False)
  np.testing.assert_array_equal(cnts.cpu().numpy(), 2 * want_c)
  assert np.all(np.abs(sums.cpu().numpy() - 2 * s1) <= 1e-13 * scale * max(1, N) ** 0.5 + 1e-300)


def _assign_case(kind, dt):
  g = np.random.default_rng(zlib.crc32(kind.encode()))  # hash() of a str varies per process
  if kind == 'uniform':
    pts = g.random((20000, 128)).astype(dt); C = pts[:256].astype(np.float64)
  elif kind == 'ties':                      # duplicate centres + exact midpoints
    C = g.random((64, 24)); C[40] = C[3]; C[41] = C[3]
    pts = g.random((6000, 24)).astype(dt)
    for i in range(0, 6000, 7):
      a, b = g.integers(0, 64, 2)
      pts[i] = ((C[a] + C[b]) / 2).astype(dt)
    pts[1::11] = C[g.integers(0, 64, len(pts[1::11]))].astype(dt)
  elif kind == 'offset':                    # |p|^2 >> d^2: stresses the bound
    C = 1e4 + g.random((300, 40)); pts = (1e4 + g.random((5000, 40))).astype(dt)
  elif kind == 'clusters':                  # tight clusters, many near-equidistant
    ctr = g.random((20, 33)) * 10
    pts = (ctr[g.integers(0, 20, 8000)] + 1e-3 * g.standard_normal((8000, 33))).astype(dt)
    C = ctr[g.integers(0, 20, 517)] + 1e-3 * g.standard_normal((517, 33))
  elif kind == 'k1':
    C = g.random((1, 7)); pts = g.random((1000, 7)).astype(dt)
  elif kind == 'nonfinite':
    C = g.random((30, 16)); pts = g.random((3000, 16)).astype(dt)
    pts[5, 3] = np.nan; pts[9, 0] = np.inf; pts[13, :] = -np.inf
  elif kind == 'ties32':                    # centres 1e-9 apart: distinct in fp64, equal once rounded to fp32
    C = g.random((256, 128)); C[200] = C[7]; C[200, 5] += 1e-9; C[31] = C[250]; C[250, 0] -= 1e-9
    pts = g.random((40000, 128)).astype(dt)
    pts[::5] = (C[7] + 0.01 * g.standard_normal((len(pts[::5]), 128))).astype(dt)
    pts[1::5] = (C[250] + 0.01 * g.standard_normal((len(pts[1::5]), 128))).astype(dt)
  return np.ascontiguousarray(pts), np.ascontiguousarray(C)


@pytest.mark.parametrize('ddt', [np.float64, np.float32])
@pytest.mark.parametrize('dt', [np.float32, np.float64])
@pytest.mark.parametrize('kind', ['uniform', 'ties', 'offset', 'clusters', 'k1', 'nonfinite', 'ties32'])
def test_kmeans_assign_certified_bit_exact(ex, kind, dt, ddt):
  """The MFMA-certified fast path must give argmin(scipy cdist) bit for bit
  (first index on ties, NaN rows -> first NaN = 0), identical to the
  all-exact kernel; with ddt float32 the argmin of the distances rounded to
  fp32 (an fp32 outer-product target), whose ties the rounding creates."""
  import torch
  from scipy.spatial.distance import cdist
  from spartan_amd import backend
  be = backend.get()
  pts, C = _assign_case(kind, dt)
  want = cdist(pts.astype(np.float64), C).astype(ddt).argmin(1)
  P = torch.as_tensor(pts).cuda()
  Cd = torch.as_tensor(C).cuda()
  fast = torch.empty(len(pts), dtype=torch.int64, device='cuda')
  slow = torch.empty_like(fast)
  be.kmeans_assign(P, Cd, fast, dist_dtype=ddt)
  be.kmeans_assign(P, Cd, slow, exact_only=True, dist_dtype=ddt)
  np.testing.assert_array_equal(slow.cpu().numpy(), want)
  np.testing.assert_array_equal(fast.cpu().numpy(), want)
  if kind == 'ties32':  # the case is only a test if the two orders differ
    want64 = cdist(pts.astype(np.float64), C).argmin(1)
    assert (want64 != cdist(pts.astype(np.float64), C).astype(np.float32).argmin(1)).any()


def _first_pass(be, mode, P, C, out, ddt=np.float64):
  """Labels through one of the two certified first passes: 'assign' -- the
  A-stationary fp16 screen of spx_kmeans_assign; 'step' -- the B-stationary
  fused screen + accumulation of spx_kmeans_step.  Both end in the same list
  passes (bf16x3, candidate masks, exact recompute)."""
  import torch
  if mode == 'assign':
    be.kmeans_assign(P, C, out, dist_dtype=ddt)
  else:
    K, D = C.shape
    sums = torch.empty((K, D), dtype=torch.float64, device=P.device)
    cnt = torch.empty((K,), dtype=torch.int64, device=P.device)
    be.kmeans_step(P, C, out, sums, cnt, dist_dtype=ddt)


@pytest.mark.parametrize('mode', ['assign', 'step'])
@pytest.mark.parametrize('D', [64, 128])
@pytest.mark.parametrize('K', [1, 7, 32, 33, 100, 256])
def test_kmeans_bf16x3_filter_bit_exact(ex, D, K, mode):
  """The certified filters (fp32 points, K <= 256, D in {64, 128}) behind
  both first passes (the A-stationary screen of spx_kmeans_assign and the
  fused B-stationary screen of spx_kmeans_step): labels bit-identical to the
  all-exact fp64 kernel (scipy cdist order, ties -> first index) on uniform
  data, exact duplicate centres, equidistant points, a ragged last tile, rows
  that must take the non-finite path (NaN, 1e30), a component past the fp16
  range (7e4) and rows in the fp16 subnormal range."""
  import torch
  from oracle import workloads as OW
  from spartan_amd import backend
  be = backend.get()
  g = np.random.default_rng(D * 1000 + K)
  n = 20011
  pts = g.random((n, D)).astype(np.float32)
  centers = pts[g.choice(n, K, replace=False)].astype(np.float64)
  if K >= 4:
    centers[K - 1] = centers[0]                                   # duplicate centre
    pts[5] = ((centers[1] + centers[2]) / 2).astype(np.float32)   # near-equidistant
    pts[6] = centers[3].astype(np.float32)                        # on a centre
  pts[7] = np.nan
  pts[8, 3] = 1e30
  pts[9] = -pts[10]
  pts[11, 5] = 7e4                  # finite in fp32, inf in fp16
  pts[12] *= np.float32(1e-6)       # fp16 subnormals
  pts[13] = 0.0
  P = torch.as_tensor(pts).cuda()
  C = torch.as_tensor(centers).cuda()
  fast = torch.empty(n, dtype=torch.int64, device='cuda')
  exact = torch.empty(n, dtype=torch.int64, device='cuda')
  _first_pass(be, mode, P, C, fast)
  be.kmeans_assign(P, C, exact, exact_only=True)
  f, e = fast.cpu().numpy(), exact.cpu().numpy()
  np.testing.assert_array_equal(f, e)
  ok = np.isfinite(pts).all(1)
  np.testing.assert_array_equal(f[ok][:3000], OW.kmeans_assign(pts[ok][:3000], centers))


@pytest.mark.parametrize('mode', ['assign', 'step'])
@pytest.mark.parametrize('ddt', [np.float64, np.float32])
@pytest.mark.parametrize('kind', ['offset128', 'means', 'clusters64', 'negative', 'wide'])
def test_kmeans_centred_filters_bit_exact(ex, kind, ddt, mode):
  """Both bf16x3 filters rank centres by cc - 2 x.c' with c' = c - mean(c)
  (kmeans_kernels.h k_kmeans_prep_b3): labels stay bit-identical to argmin(cdist) for
  data far from the origin (the case centring is for), second-iteration
  centres (cluster means, the tight-gap case), tight clusters and negative
  coordinates, in both filter modes and both distance dtypes."""
  import torch
  from scipy.spatial.distance import cdist
  from spartan_amd import backend
  be = backend.get()
  g = np.random.default_rng(zlib.crc32(kind.encode()))
  if kind == 'offset128':
    pts = (1e3 + g.random((30011, 128))).astype(np.float32)
    C = pts[:256].astype(np.float64)
  elif kind == 'means':
    pts = g.random((30011, 128)).astype(np.float32)
    C0 = pts[:256].astype(np.float64)
    lab = cdist(pts.astype(np.float64), C0).argmin(1)
    C = np.stack([pts[lab == k].astype(np.float64).mean(0) if (lab == k).any() else C0[k] for k in range(256)])
  elif kind == 'clusters64':
    ctr = g.random((40, 64)) * 5
    pts = (ctr[g.integers(0, 40, 20000)] + 1e-2 * g.standard_normal((20000, 64))).astype(np.float32)
    C = ctr[g.integers(0, 40, 200)] + 1e-2 * g.standard_normal((200, 64))
  elif kind == 'wide':  # centres beyond the fp16 range: the screen passes every row on
    pts = (g.random((20000, 128)) * 1e5).astype(np.float32)
    C = pts[g.choice(20000, 150, replace=False)].astype(np.float64)
  else:
    pts = (g.standard_normal((20000, 128)) * 3 - 7).astype(np.float32)
    C = pts[g.choice(20000, 97, replace=False)].astype(np.float64)
  want = cdist(pts.astype(np.float64), C).astype(ddt).argmin(1)
  P = torch.as_tensor(pts).cuda()
  Cd = torch.as_tensor(np.ascontiguousarray(C)).cuda()
  fast = torch.empty(len(pts), dtype=torch.int64, device='cuda')
  _first_pass(be, mode, P, Cd, fast, ddt)
  np.testing.assert_array_equal(fast.cpu().numpy(), want)


# ---------------------------------------------- views: slice / transpose / reshape
@pytest.mark.parametrize('W', [1, 3])
def test_views_gpu(ex, W):
  """The reference's test_slice / test_transpose / test_reshape cases through
  the gfx950 kernels: slices and transposes are zero-copy views whose pieces
  the generated kernels read in place (transposes as strided operands);
  reshape is one gather + copy-region pass."""
  from test_views import _views_cases
  expr, setw = ex
  setw(W)
  for name, e, want in _views_cases(expr):
    got = e.glom()
    np.testing.assert_allclose(np.asarray(got).reshape(np.shape(want)), want, rtol=1e-12, err_msg=name)


# ---------------------------------------------- writes / ingest / egress (8(f) rank 3)
@pytest.mark.parametrize('W', [1, 3])
def test_write_gpu(ex, W, tmp_path):
  """The reference's test_write cases, sub-region merges with reducers
  (spx_merge masked and unmasked paths), self-aliasing writes and writes
  from transposed views, on the GPU."""
  from test_write import _run_write_cases
  expr, setw = ex
  setw(W)
  _run_write_cases(expr, str(tmp_path))


def test_transfer_pipeline_gpu(ex, tmp_path):
  """Pinned double-buffered upload / download (array/transfer.py) at sizes
  that take the pipeline: strided host pieces, a memmap, rows wider than a
  staging block, bool and int dtypes, strided download targets."""
  import torch
  from spartan_amd.array import transfer
  expr, setw = ex
  setw(1)
  dev = torch.device('cuda:0')
  big = rng.rand((3000, 2000), 31, np.float32)            # 24 MB: two staging blocks
  for piece in (big, big[:, 500:1700], big[1:2999:2, ::3], big.T):
    t = transfer.upload(piece, dev)
    np.testing.assert_array_equal(t.cpu().numpy(), piece)
    np.testing.assert_array_equal(transfer.download(t), piece)
    out = np.zeros((piece.shape[0], piece.shape[1] + 7), np.float32)
    transfer.download(t, out[:, 3:3 + piece.shape[1]])
    np.testing.assert_array_equal(out[:, 3:3 + piece.shape[1]], piece)
    assert not out[:, :3].any() and not out[:, 3 + piece.shape[1]:].any()
  wide = rng.rand((3, transfer.CHUNK // 8 + 5), 32, np.float64)  # rows wider than a block
  t = transfer.upload(wide, dev)
  np.testing.assert_array_equal(transfer.download(t), wide)
  out = np.zeros((3, wide.shape[1] + 1))
  transfer.download(t, out[:, 1:])
  np.testing.assert_array_equal(out[:, 1:], wide)
  flags = (rng.rand((5_000_000,), 33, np.float64) > 0.5)
  np.testing.assert_array_equal(transfer.download(transfer.upload(flags, dev)), flags)
  ints = np.arange(3_000_000, dtype=np.int64).reshape(1000, 3000)
  np.testing.assert_array_equal(transfer.download(transfer.upload(ints, dev)), ints)
  fn = str(tmp_path / 'm.npy')
  np.save(fn, big)
  mm = np.load(fn, mmap_mode='r')
  x = expr.from_file(fn)
  np.testing.assert_array_equal(x.glom(), big)
  np.testing.assert_allclose(x.sum(0).glom(), big.astype(np.float64).sum(0), rtol=1e-5)
  del mm


# ---------------------------------------------- joins: map2 / outer (8(f) rank 4)
@pytest.mark.parametrize('W', [1, 3])
def test_join_gpu(ex, W):
  """The reference's k-means mappers through expr.outer / map2 (spx_cdist,
  spx_bincount, spx_kmeans_accumulate), the fused argmin (spx_kmeans_assign),
  bincount / concatenate and traced elementwise joins, on the GPU."""
  from test_join import _run_join_cases
  from spartan_amd.config import FLAGS
  expr, setw = ex
  setw(W)
  _run_join_cases(expr, FLAGS)


def test_cdist_and_fused_kmeans_gpu(ex):
  """spx_cdist bit-exact against scipy at a size that spans many 64 x 64
  tiles and a D that is not a multiple of the 16-dim chunk; the unmodified
  KMeans driver on fp32 points with D % 64 == 0 (the certified bf16x3 filter
  inside the fused argmin) against the oracle."""
  from scipy.spatial.distance import cdist
  from spartan_amd.examples.kmeans import KMeans, kmeans_dist_mapper
  from test_join import _kmeans_oracle
  expr, setw = ex
  setw(2)
  X = rng.rand((3001, 37), 61, np.float64)
  C = rng.rand((130, 37), 62, np.float64)
  d = expr.outer((expr.from_numpy(X), expr.from_numpy(C)), (0, 0), fn=kmeans_dist_mapper, shape=(3001, 130))
  np.testing.assert_array_equal(d.glom(), cdist(X, C))
  X32 = rng.rand((40000, 64), 63, np.float32)
  c0 = X32[:48].astype(np.float64)
  got_c, got_l = KMeans(48, 3).fit(expr.from_numpy(X32), centers=c0)
  wc, wl = _kmeans_oracle(X32, c0, 3, center_dtype=np.float32)
  np.testing.assert_array_equal(got_l.glom(), wl)
  np.testing.assert_allclose(got_c, wc, rtol=1e-6)


@pytest.mark.parametrize('W', [1, 3])
def test_location_gpu(ex, W):
  """map_with_location (per-tile traced kernels) and region_map on the GPU."""
  from test_location import _run_location_cases
  expr, setw = ex
  setw(W)
  _run_location_cases(expr, W)


def test_multirank_rehearsal_gpu(tmp_path):
  """N = 2 ranks on this one GPU (torchrun, gloo with host staging): the
  multi-rank tile plans, exchanges and combines with the real kernels."""
  import subprocess
  import socket
  s = socket.socket()
  s.bind(('127.0.0.1', 0))
  port = s.getsockname()[1]
  s.close()
  env = dict(os.environ, SPARTAN_DIST_BACKEND='gloo', REHEARSAL_WORKERS='3')
  cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node=2',
         '--master-addr=127.0.0.1', '--master-port=%d' % port, os.path.join(HERE, 'mrank_body.py')]
  r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=240)
  assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
  assert r.stdout.count('rehearsal ok') == 2, r.stdout[-2000:]


def test_bench_two_ranks_gpu():
  """bench.py --gpus 2 --full as the driver's scaling sweep starts it by
  hand: no RANK in the environment, so bench.py launches its own two ranks
  (launch_ranks -> torch.distributed.run) and relays rank 0's line.  Both
  ranks share this box's one GPU, so the data plane is the gloo rehearsal
  (SPARTAN_DIST_BACKEND=gloo; RCCL refuses two ranks on one device); every
  leg runs at small sizes and validates its own outputs.  Reference harness:
  tests/test_common.py:102-121 (worker-count sweep)."""
  import json
  import subprocess
  env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
  env.update(SPARTAN_DIST_BACKEND='gloo', SPARTAN_SPMD_GUARD='strict')
  cmd = [sys.executable, os.path.join(os.path.dirname(HERE), 'bench.py'), '--gpus', '2', '--full', '--size', '4096',
         '--steps', '2', '--warmup', '1', '--dot-size', '2048', '--km-points', '200000', '--lreg-points',
         '200000', '--cpu-baseline', '0']
  r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=280)
  assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
  lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
  assert len(lines) == 1, r.stdout[-3000:]
  d = json.loads(lines[0])
  assert d['n_gpus'] == 2 and d['n_ranks_seen'] == 2 and d['scaling'] == 'weak'
  assert d['config']['shape'] == [8192, 4096]   # weak scaling: one 4096-row strip per rank
  assert d['checked'] is True
  # round 6: the default multi-rank data plane is self-tested at start-up and
  # its process group carries a bounded timeout
  assert d['dataplane_selftest'] == 'ok' and d['pg_timeout_s'] == 300.0
  for leg in ('lreg', 'kmeans', 'kmeans_api'):
    assert d[leg].get('checked') is True, (leg, d[leg])
  for dt in ('f32', 'f64'):
    assert d['dot'][dt]['checked'] is True, d['dot']


def test_bench_plain_run_dumps_outputs_gpu(tmp_path):
  """A plain bench.py run (no --full) times exactly --steps steps, prints the
  headline line without any of the --full legs, and --dump-outputs writes the
  last step's axis-0 / axis-1 sums as float32 .npy: the same from run to run,
  and within 1e-5 (the fp32 bound) of fp64 sums of the same fp32 inputs."""
  import json
  import subprocess
  env = {k: v for k, v in os.environ.items() if k not in ('RANK', 'WORLD_SIZE', 'LOCAL_RANK')}
  S = 512
  got = []
  for name in ('a', 'b'):
    out = str(tmp_path / name)
    cmd = [sys.executable, os.path.join(os.path.dirname(HERE), 'bench.py'), '--gpus', '1', '--size', str(S),
           '--steps', '3', '--warmup', '1', '--dump-outputs', out]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, r.stdout[-3000:]
    d = json.loads(lines[0])
    assert d['steps'] == 3 and d['warmup'] == 1 and d['ms_per_step'] > 0
    assert d['unit'] == 'GB/s' and d['higher_is_better'] is True and d['dtype'] == 'f32'
    # value = algorithmic bytes of the 3 timed steps / their wall time (the line
    # rounds ms_per_step to 1e-4 ms: under 1e-2 relative for any step over 5 us)
    total = 2 * (3 * 4 * S * S + 4 * S) * 3
    assert d['value'] == pytest.approx(total / (d['ms_per_step'] * 3 * 1e-3) / 1e9, rel=1e-2, abs=0.02)
    for leg in ('checked', 'cold_start', 'cfg2_axis_none', 'cfg2_map', 'vendor_reduce', 'dot', 'lreg', 'kmeans',
                'kmeans_api', 'cpu_baseline'):
      assert leg not in d, leg
    assert sorted(os.listdir(out)) == ['axis0.npy', 'axis1.npy']
    got.append([np.load(os.path.join(out, f)) for f in ('axis0.npy', 'axis1.npy')])
  x, y = (rng.rand((S, S), s, np.float32).astype(np.float64) for s in (11, 12))
  z = rng.rand((S, S), 13, np.float32, -1.0, 1.0).astype(np.float64)
  m = x * y + np.exp(z)
  for axis in (0, 1):
    assert got[0][axis].dtype == np.float32 and got[0][axis].shape == (S,)
    np.testing.assert_array_equal(got[0][axis], got[1][axis])
    np.testing.assert_allclose(got[0][axis], m.sum(axis), rtol=1e-5)


@pytest.mark.parametrize('W', [1, 3])
def test_nonfinite_reductions(ex, W):
  """NaN / +-inf through sum / min / max / argmin / argmax, across tiles:
  NaN propagates as in np.minimum / np.maximum (the reference's accumulate
  functions), arg-reductions return the first NaN (numpy's rule)."""
  expr, setw = ex
  setw(W)
  a = rng.rand((37, 23), 71, np.float32)
  a[3, 5] = np.nan
  a[20, 7] = np.inf
  a[30, 11] = -np.inf
  a[31, 5] = np.nan
  A = expr.from_numpy(a)
  for axis in (None, 0, 1):
    np.testing.assert_array_equal(expr.min(A, axis).glom(), np.min(a, axis))
    np.testing.assert_array_equal(expr.max(A, axis).glom(), np.max(a, axis))
    np.testing.assert_array_equal(A.argmin(axis).glom(), a.argmin(axis))
    np.testing.assert_array_equal(A.argmax(axis).glom(), a.argmax(axis))
    got = np.asarray(expr.sum(A, axis).glom(), dtype=np.float64)
    want = np.sum(a.astype(np.float64), axis)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
  b = rng.rand((37, 23), 72, np.float64)
  b[:, 4] = np.inf
  b[9, 4] = -np.inf
  B = expr.from_numpy(b)
  for axis in (None, 0, 1):
    got = np.asarray(expr.sum(B, axis).glom())
    want = np.sum(b, axis)
    np.testing.assert_array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_array_equal(np.isinf(got), np.isinf(want))
    np.testing.assert_array_equal(A.argmin(axis).glom(), a.argmin(axis))


@pytest.mark.parametrize('limit', [None, 4096])
def test_broadcast_reduce_views(ex, limit):
  """Reductions whose inputs broadcast along different dims ((N,1,D) - (1,K,D)
  and friends): materialised then reduced, whole or -- above the byte limit
  -- in slabs of a kept dim; every axis, sum and argmin."""
  from spartan_amd import backend
  expr, setw = ex
  setw(2)
  be = backend.get()
  old = be.MATERIALISE_LIMIT
  if limit is not None:
    be.MATERIALISE_LIMIT = limit
  try:
    X = rng.rand((50, 6), 81, np.float64)
    C = rng.rand((7, 6), 82, np.float64)
    Xb = expr.reshape(expr.from_numpy(X), (50, 1, 6))
    Cb = expr.reshape(expr.from_numpy(C), (1, 7, 6))
    d3 = (X[:, None, :] - C[None, :, :]) ** 2
    for axis in (0, 1, 2):
      np.testing.assert_allclose(expr.sum(expr.square(Xb - Cb), axis=axis).optimized().glom(), d3.sum(axis),
                                 rtol=1e-12)
      np.testing.assert_array_equal(expr.argmin(expr.square(Xb - Cb), axis=axis).optimized().glom(),
                                    d3.argmin(axis))
  finally:
    be.MATERIALISE_LIMIT = old


@pytest.mark.parametrize('W', [1, 3])
def test_optimization_dags_gpu(ex, W):
  """tests/test_optimization.py's nonordered / reduced DAGs at the reference's
  size (1000 x 1000 fp64): slices of fused maps, a dot of slices, a sum."""
  from test_views import _optimization_dag_cases
  expr, setw = ex
  setw(W)
  for name, e, want in _optimization_dag_cases(expr, 1000):
    np.testing.assert_allclose(e.optimized().glom(), want, rtol=1e-10, err_msg=name)


@pytest.mark.parametrize('W', WORKERS)
def test_dot_forced_operands_gpu(ex, W):
  """dot() of forced DistArrays (device operands, no host round trip)."""
  expr, setw = ex
  setw(W)
  for dt in (np.float32, np.float64):
    a = expr.rand(96, 160, dtype=dt, seed=3).force()
    b = expr.rand(160, 72, dtype=dt, seed=4).force()
    na, nb = rng.rand((96, 160), 3, dt), rng.rand((160, 72), 4, dt)
    exact = na.astype(np.float64) @ nb.astype(np.float64)
    check_fp(expr.dot(a, b).glom(), O.dot_tiles(na, nb, W), exact, 1e-5 if dt == np.float32 else 1e-12)


@pytest.mark.parametrize('W', WORKERS)
def test_map_forced_operands_gpu(ex, W):
  """Fused map / reduce over forced DistArrays (one operand each)."""
  expr, setw = ex
  setw(W)
  a = expr.rand(130, 70, dtype=np.float32, seed=5).force()
  na = rng.rand((130, 70), 5, np.float32)
  np.testing.assert_allclose(expr.exp(a).glom(), np.exp(na), rtol=1e-6)
  np.testing.assert_array_equal(expr.map((a, a), np.multiply).glom(), na * na)
  got = expr.sum(expr.map(a, np.sqrt), axis=0).optimized().glom()
  mapped = np.sqrt(na)
  check_fp(got, O.sum_tiles(mapped, 0, W), mapped.astype(np.float64).sum(0), 1e-5)


def test_rccl_single_rank_collectives(ex):
  """Every libspx collective on a one-rank RCCL communicator (the only
  communicator one GPU can hold): dtype / op mapping, stream order, in-place
  and out-of-place buffers, grouped point-to-point to self.  The N-rank
  decomposition logic above it is the gloo world-2 tests' (same comm.py
  call sites)."""
  import ctypes
  import torch
  from spartan_amd import comm
  lib = comm._lib()
  uid = comm.rccl_unique_id()
  c = comm.rccl_init(0, 1, uid)
  try:
    dev = torch.device('cuda', torch.cuda.current_device())
    st = comm._stream()
    for dt in (torch.float32, torch.float64, torch.int64, torch.int32):
      x = (torch.arange(1000, device=dev) * 3 - 7).to(dt)
      y = torch.empty_like(x)
      for op in (0, 1, 2):
        assert lib.spx_allreduce(c, comm._p(x), comm._p(y), x.numel(), comm._dt(x), op, st) == 0
        torch.cuda.synchronize()
        assert torch.equal(x, y)
      assert lib.spx_reduce_scatter(c, comm._p(x), comm._p(y), x.numel(), comm._dt(x), 0, st) == 0
      g = torch.empty((1, 1000), dtype=dt, device=dev)
      assert lib.spx_allgather(c, comm._p(x), comm._p(g), x.numel(), comm._dt(x), st) == 0
      z = x.clone()
      assert lib.spx_broadcast(c, comm._p(z), comm._p(z), z.numel(), comm._dt(z), 0, st) == 0
      r = torch.empty_like(x)
      assert lib.spx_reduce(c, comm._p(x), comm._p(r), x.numel(), comm._dt(x), 0, 0, st) == 0
      torch.cuda.synchronize()
      assert torch.equal(y, x) and torch.equal(g[0], x) and torch.equal(z, x) and torch.equal(r, x)
    a = torch.arange(257, dtype=torch.float64, device=dev)
    b = torch.zeros_like(a)
    VP, I64, I32 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int
    rc = lib.spx_sendrecv(c, 1, (VP * 1)(a.data_ptr()), (I64 * 1)(a.numel() * 8), (I32 * 1)(0),
                          1, (VP * 1)(b.data_ptr()), (I64 * 1)(b.numel() * 8), (I32 * 1)(0), st)
    assert rc == 0, lib.spx_last_error()
    torch.cuda.synchronize()
    assert torch.equal(a, b)
  finally:
    torch.cuda.synchronize()
    comm.rccl_destroy(c)


@pytest.mark.parametrize('W', [1, 3])
def test_untraceable_mappers_gpu(ex, W):
  """User mappers that cannot become a kernel (np.sort on the tile, a Python
  branch on the tile's values) run per tile on the host as the reference
  runs every mapper (local.py:110-122); counted, and results equal NumPy's.
  A reduction over such a mapper reduces the uploaded tiles on the GPU."""
  import warnings
  expr, setw = ex
  setw(W)
  from spartan_amd.expr import engine
  from spartan_amd.array import distarray
  a = (rng.rand((300, 50), 5, np.float64) * 10.0).round()
  x = expr.from_numpy(a)
  tiles = sorted(distarray.from_numpy(a).tiles, key=lambda e: e.ul)
  strips = [a[e.ul[0]:e.lr[0]] for e in tiles]

  def branchy(t):
    if t.sum() > 100 * t.shape[0] * 5:
      return t * 2.0
    return t - 1.0

  n0 = engine.HOST_MAPPER_CALLS[0]
  with warnings.catch_warnings():
    warnings.simplefilter('ignore', RuntimeWarning)
    np.testing.assert_array_equal(expr.map(x, lambda t: np.sort(t, axis=1)).glom(), np.sort(a, axis=1))
    want = np.concatenate([branchy(s) for s in strips])
    np.testing.assert_array_equal(expr.map(x, branchy).glom(), want)
    np.testing.assert_allclose(expr.sum(expr.map(x, branchy), axis=0).optimized().glom(), want.sum(0),
                               rtol=1e-12)
  assert engine.HOST_MAPPER_CALLS[0] - n0 == 3 * len(tiles)
  n1 = engine.HOST_MAPPER_CALLS[0]
  np.testing.assert_allclose(expr.map(x, lambda t: t * t + 1.0).glom(), a * a + 1.0, rtol=1e-15)
  assert engine.HOST_MAPPER_CALLS[0] == n1   # traceable: a generated kernel


# ------------------------------------------ fused k-means step (one pass)
def _step_case(kind):
  g = np.random.default_rng(zlib.crc32(('step-' + kind).encode()))
  if kind in ('uniform', 'ties32'):
    return _assign_case(kind, np.float32)
  if kind == 'd64':          # D = 64, K = 256, N not a multiple of 32
    pts = g.random((50003, 64)).astype(np.float32); C = pts[:256].astype(np.float64)
  elif kind == 'k20':        # one centre tile (NCT = 1), padding centres
    pts = g.random((7001, 128)).astype(np.float32); C = g.random((20, 128))
  elif kind == 'k50':        # NCT = 2
    pts = g.random((9000, 64)).astype(np.float32); C = g.random((50, 64))
  elif kind == 'k100':       # NCT = 4, tight clusters (many undecided rows)
    ctr = g.random((100, 128)) * 2
    pts = (ctr[g.integers(0, 100, 12000)] + 1e-3 * g.standard_normal((12000, 128))).astype(np.float32)
    C = ctr + 1e-3 * g.standard_normal((100, 128))
  elif kind == 'k1':
    pts = g.random((3000, 64)).astype(np.float32); C = g.random((1, 64))
  elif kind == 'nonfinite':
    pts = g.random((8000, 128)).astype(np.float32); C = g.random((256, 128))
    pts[5, 3] = np.nan; pts[9, 0] = np.inf; pts[4000, :] = -np.inf; pts[77, 1] = 7e4  # fp16 overflow
  elif kind == 'tiny':       # fewer tiles than blocks
    pts = g.random((45, 128)).astype(np.float32); C = pts[:7].astype(np.float64)
  return np.ascontiguousarray(pts), np.ascontiguousarray(C)


@pytest.mark.parametrize('ddt', [np.float64, np.float32])
@pytest.mark.parametrize('kind', ['uniform', 'ties32', 'd64', 'k20', 'k50', 'k100', 'k1', 'nonfinite', 'tiny'])
def test_kmeans_step_matches_two_passes(ex, kind, ddt):
  """spx_kmeans_step (the fused screen + accumulation) against the two-pass
  path: labels bit-identical to spx_kmeans_assign and to the all-exact kernel
  (scipy cdist order, first index); counts exact; sums within the fp32 rule
  of the fp64-exact sums (1e-5 of sum |x| per element: the rows the screen
  decides are summed in fp32 per block and window of 256 64-row units, the
  windows then in fp64; the reference sums in fp32, k_means_.py:67-89);
  repeated runs bit-identical;
  zero_first=False adds."""
  import torch
  from spartan_amd import backend
  be = backend.get()
  pts, C = _step_case(kind)
  N, D = pts.shape
  K = C.shape[0]
  P = torch.as_tensor(pts).cuda()
  Cd = torch.as_tensor(C).cuda()
  lab = torch.empty((N,), dtype=torch.int64, device='cuda')
  sums = torch.full((K, D), 5.0, dtype=torch.float64, device='cuda')
  cnt = torch.full((K,), 9, dtype=torch.int64, device='cuda')
  be.kmeans_step(P, Cd, lab, sums, cnt, zero_first=True, dist_dtype=ddt)
  if kind in ('uniform', 'd64'):
    # the fused screen does decide: well-separated rows never reach the list
    # passes (a screen that decides nothing is still exact, only slow)
    und = be.kmeans_counters(D)[3]
    assert und <= 0.2 * N, 'fused screen left %d of %d rows undecided' % (und, N)
  want = torch.empty_like(lab)
  be.kmeans_assign(P, Cd, want, dist_dtype=ddt)
  exact = torch.empty_like(lab)
  be.kmeans_assign(P, Cd, exact, exact_only=True, dist_dtype=ddt)
  assert torch.equal(want, exact)
  assert torch.equal(lab, exact)
  L = lab.cpu().numpy()
  ok = (L >= 0) & (L < K)
  np.testing.assert_array_equal(cnt.cpu().numpy(), np.bincount(L[ok], minlength=K))
  ws = np.zeros((K, D))
  wa = np.zeros((K, D))
  p64 = pts.astype(np.float64)
  np.add.at(ws, L[ok], p64[ok])
  np.add.at(wa, L[ok], np.abs(p64[ok]))
  s1 = sums.cpu().numpy().copy()
  fin = np.isfinite(ws)
  assert np.all(np.abs(s1[fin] - ws[fin]) <= 1e-5 * wa[fin] + 1e-300)
  assert np.array_equal(np.isnan(s1), np.isnan(ws))
  be.kmeans_step(P, Cd, lab, sums, cnt, zero_first=True, dist_dtype=ddt)
  np.testing.assert_array_equal(sums.cpu().numpy(), s1)   # deterministic
  be.kmeans_step(P, Cd, lab, sums, cnt, zero_first=False, dist_dtype=ddt)
  np.testing.assert_array_equal(cnt.cpu().numpy(), 2 * np.bincount(L[ok], minlength=K))
  s2 = sums.cpu().numpy()
  assert np.all(np.abs(s2[fin] - 2 * ws[fin]) <= 2e-5 * wa[fin] + 1e-300)


def test_kmeans_step_windows(ex):
  """Enough rows that every block passes several 504-unit windows (the fp32
  sums written to the block's window slots and cleared inside the unit
  loop): 12M x 64 = 1465 32-row units per block on 256 CUs."""
  import torch
  from spartan_amd import backend
  be = backend.get()
  N, D, K = 12_000_000, 64, 256
  P = torch.empty((N, D), dtype=torch.float32, device='cuda')
  be.fill(P, backend.FILL_UNIFORM, 0.0, 1.0, 77, (0, 0), (N, D))
  Cd = P[1000:1000 + K].to(torch.float64).contiguous()
  lab = torch.empty((N,), dtype=torch.int64, device='cuda')
  sums = torch.empty((K, D), dtype=torch.float64, device='cuda')
  cnt = torch.empty((K,), dtype=torch.int64, device='cuda')
  be.kmeans_step(P, Cd, lab, sums, cnt)
  exact = torch.empty_like(lab)
  be.kmeans_assign(P, Cd, exact, exact_only=True)
  assert torch.equal(lab, exact)
  assert torch.equal(cnt, torch.bincount(lab, minlength=K))
  torch.testing.assert_close(sums, _centre_sums64(lab, P, K), rtol=1e-5, atol=0)  # the fp32 rule (points >= 0)
  # the window slots were used: a block's 32-row units span several flushes
  assert (N + 31) // 32 // 256 > 2 * 504


def test_kmeans_step_workspace_base_16_aligned(ex):
  """spx_kmeans_step through the raw ABI with a workspace base that is 16-byte
  but not 256-byte aligned, and exactly spx_kmeans_step_workspace bytes behind
  it: the size function budgets the padding of every field the layout aligns
  on its absolute address.  Labels, sums and counts equal the aligned run's
  bit for bit."""
  import ctypes
  import torch
  from spartan_amd import backend
  be = backend.get()
  N, D, K = 4097, 64, 33
  P = torch.empty((N, D), dtype=torch.float32, device='cuda')
  be.fill(P, backend.FILL_UNIFORM, 0.0, 1.0, 5, (0, 0), (N, D))
  Cd = P[:K].to(torch.float64).contiguous()
  need = int(be.lib.spx_kmeans_step_workspace(backend.SPX_F32, N, D, K))
  assert need > 0
  ws = torch.empty((need + 16,), dtype=torch.uint8, device='cuda')
  assert ws.data_ptr() % 256 == 0
  got = []
  for shift in (0, 16):
    lab = torch.full((N,), -7, dtype=torch.int64, device='cuda')
    sums = torch.empty((K, D), dtype=torch.float64, device='cuda')
    cnt = torch.empty((K,), dtype=torch.int64, device='cuda')
    rc = be.lib.spx_kmeans_step(backend.SPX_F32, N, D, K, ctypes.c_void_p(P.data_ptr()), P.stride(0),
                                ctypes.c_void_p(Cd.data_ptr()), ctypes.c_void_p(lab.data_ptr()),
                                ctypes.c_void_p(sums.data_ptr()), ctypes.c_void_p(cnt.data_ptr()), 1,
                                ctypes.c_void_p(ws.data_ptr() + shift), need, backend.SPX_F64, be.stream())
    assert rc == 0, be.lib.spx_last_error()
    torch.cuda.synchronize()
    got.append((lab, sums, cnt))
  for a, b in zip(*got):
    assert torch.equal(a, b)
  assert int(got[0][2].sum()) == N and int(got[0][0].min()) >= 0


def _centre_sums64(lab, X, K, chunk=1 << 20):
  """Checker: per-centre fp64 sums of the rows of X by label, as a one-hot
  fp64 GEMM per chunk of rows (torch, test-only).  index_add_ would be the
  obvious form, but its fp64 atomics serialise when most rows share a label
  (the skewed cases below: minutes for 12M rows)."""
  import torch
  out = torch.zeros((K, X.shape[1]), dtype=torch.float64, device=X.device)
  for r0 in range(0, X.shape[0], chunk):
    oh = torch.nn.functional.one_hot(lab[r0:r0 + chunk], K).to(torch.float64)
    out += oh.t() @ X[r0:r0 + chunk].to(torch.float64)
  return out


def _step_check_all(be, P, Cd, rtol=1e-5):
  """spx_kmeans_step on (P, Cd): labels equal the all-exact kernel's, counts
  equal the bincount of them, sums within rtol of the fp64 index-add (points
  >= 0, so sum |x| = sum x)."""
  import torch
  N, D = P.shape
  K = Cd.shape[0]
  lab = torch.empty((N,), dtype=torch.int64, device='cuda')
  sums = torch.empty((K, D), dtype=torch.float64, device='cuda')
  cnt = torch.empty((K,), dtype=torch.int64, device='cuda')
  be.kmeans_step(P, Cd, lab, sums, cnt)
  exact = torch.empty_like(lab)
  be.kmeans_assign(P, Cd, exact, exact_only=True)
  assert torch.equal(lab, exact)
  assert torch.equal(cnt, torch.bincount(lab, minlength=K))
  torch.testing.assert_close(sums, _centre_sums64(lab, P, K), rtol=rtol, atol=0)
  return lab, cnt


@pytest.mark.parametrize('K', [2, 256])
def test_kmeans_step_long_chains(ex, K):
  """The advisory case: every window of a block puts (nearly) all of its rows
  into one or two centres, so a centre's fp32 window chain is up to 64 x 256
  rows long -- K = 2 over 12M rows, and K = 256 with 95 % of the rows next
  to centre 0 (skewed, as a first iteration from data-point centres is).
  Counts exact, labels exact, sums within 1e-5 of the fp64 sums."""
  import torch
  from spartan_amd import backend
  be = backend.get()
  N, D = 12_000_000, 64
  P = torch.empty((N, D), dtype=torch.float32, device='cuda')
  be.fill(P, backend.FILL_UNIFORM, 0.0, 1.0, 91, (0, 0), (N, D))
  if K == 2:
    Cd = torch.stack([torch.full((D,), 0.3), torch.full((D,), 0.7)]).to(torch.float64).cuda()
  else:
    P[: N * 95 // 100].mul_(0.01)  # 95 % of the rows in [0, 0.01): all nearest to centre 0
    g = np.random.default_rng(5)
    C = g.random((K, D)) * 0.5 + 0.5
    C[0] = 0.005
    Cd = torch.as_tensor(C).cuda()
  lab, cnt = _step_check_all(be, P, Cd)
  assert int(cnt.max()) > N // 2   # the chains really are long


@pytest.mark.parametrize('N', [1, 31, 63, 64, 65, 4097, 64 * 256 * 3 + 17])
def test_kmeans_step_same_row_units(ex, N):
  """Every row of every 64-row unit carries the same label (identical rows):
  the adds' table rounds take three rows of a centre and the other 61 go
  through the ranked tail loop (kmeans_kernels.h k_kmeans_fs2 add_end) -- the
  data-dependent part of the unit loop -- with ragged tails (N not a
  multiple of 64, fewer units than blocks, a single row).  Labels, counts
  and sums as the two-pass path."""
  import torch
  from spartan_amd import backend
  be = backend.get()
  D, K = 128, 256
  g = np.random.default_rng(N)
  C = g.random((K, D))
  row = (C[17] + 1e-3).astype(np.float32)
  P = torch.as_tensor(np.tile(row, (N, 1))).cuda()
  lab, cnt = _step_check_all(be, P, torch.as_tensor(C).cuda())
  assert int(cnt[17]) == N


def test_kmeans_step_far_undecided_outliers(ex):
  """a row the screen cannot decide was added provisionally to
  its screen-best centre p and moved in fp64 afterwards if its final label
  differed -- leaving the fp32 rounding of ITS add in p's window chain.  For
  a far outlier that rounding dominates p's sum.  Here 64 outliers sit
  midway between two centres a, b (final label a by a 1e-4 nudge, the fp16
  screen picks either) with a 2e4 component in one of the dims 120-127 where
  every centre and every other row is ~0 (tiny values), so element (b, d) of
  the sums has sum |x| of only ~1e-3 per row: a mover's fp32 add of 2e4 into
  it swallows every later add there (error >> 1e-5 sum |x|).  Far rows must
  stay out of the provisional adds (gathered in fp64 instead): labels exact,
  counts exact, every element within 1e-5 of the fp64 sum |x|."""
  import torch
  from spartan_amd import backend
  be = backend.get()
  g = np.random.default_rng(2024)
  N, D, K = 300_000, 128, 8
  C = np.zeros((K, D))
  C[:, :120] = g.random((K, 120))
  pts = np.zeros((N, D), dtype=np.float32)
  pts[:, :120] = g.random((N, 120))
  pts[:, 120:] = 1e-3 * g.random((N, 8))
  rows = g.choice(N, 64, replace=False)
  for i, r in enumerate(rows):
    a, b = i % K, (i + 1) % K
    mid = 0.5 * (C[a, :120] + C[b, :120]) + 1e-4 * (C[a, :120] - C[b, :120])
    pts[r, :120] = mid
    pts[r, 120 + i % 8] = 2e4
  P = torch.as_tensor(pts).cuda()
  Cd = torch.as_tensor(C).cuda()
  lab = torch.empty((N,), dtype=torch.int64, device='cuda')
  sums = torch.empty((K, D), dtype=torch.float64, device='cuda')
  cnt = torch.empty((K,), dtype=torch.int64, device='cuda')
  be.kmeans_step(P, Cd, lab, sums, cnt)
  exact = torch.empty_like(lab)
  be.kmeans_assign(P, Cd, exact, exact_only=True)
  assert torch.equal(lab, exact)
  L = lab.cpu().numpy()
  assert np.array_equal(L[rows], np.arange(64) % K)   # the nudge decides, as built
  np.testing.assert_array_equal(cnt.cpu().numpy(), np.bincount(L, minlength=K))
  p64 = pts.astype(np.float64)
  ws = np.zeros((K, D))
  wa = np.zeros((K, D))
  np.add.at(ws, L, p64)
  np.add.at(wa, L, np.abs(p64))
  s = sums.cpu().numpy()
  err = np.abs(s - ws) / wa
  assert err.max() <= 1e-5, 'max |sum - fp64| / sum |x| = %.3g at %s' % (err.max(), np.unravel_index(err.argmax(), err.shape))


@pytest.mark.parametrize('K', [1, 8, 256])
def test_kmeans_step_zero_mean_gaussian(ex, K):
  """zero-mean isotropic Gaussian rows (D = 128, |x'| ~ 11 while
  the centres' spread cmax and |mu| are far smaller for K = 1 / mean-like
  centres): the far-row cut 4 (cmax + |mu|) applies only to rows the screen
  cannot decide, so a decided far row is still added in the one pass --
  the screen's undecided fraction stays small; labels exact, counts exact,
  sums within 1e-5 of the fp64 sum |x|."""
  import torch
  from spartan_amd import backend
  be = backend.get()
  g = np.random.default_rng(606 + K)
  N, D = 200_000, 128
  pts = g.standard_normal((N, D)).astype(np.float32)
  if K == 1:
    C = np.zeros((1, D))
  else:  # centres near the mean (second-iteration-like): means of random halves of the data
    C = np.stack([pts[g.choice(N, N // 4, replace=False)].astype(np.float64).mean(0) * 8 for _ in range(K)])
  P = torch.as_tensor(pts).cuda()
  Cd = torch.as_tensor(C).cuda()
  lab = torch.empty((N,), dtype=torch.int64, device='cuda')
  sums = torch.empty((K, D), dtype=torch.float64, device='cuda')
  cnt = torch.empty((K,), dtype=torch.int64, device='cuda')
  be.kmeans_step(P, Cd, lab, sums, cnt)
  und = be.kmeans_counters(D)[3]
  print('zero-mean Gaussian K=%d: %d of %d rows undecided by the screen' % (K, und, N))
  assert und <= (0.01 if K == 1 else 0.3) * N
  exact = torch.empty_like(lab)
  be.kmeans_assign(P, Cd, exact, exact_only=True)
  assert torch.equal(lab, exact)
  L = lab.cpu().numpy()
  np.testing.assert_array_equal(cnt.cpu().numpy(), np.bincount(L, minlength=K))
  p64 = pts.astype(np.float64)
  ws = np.zeros((K, D))
  wa = np.zeros((K, D))
  np.add.at(ws, L, p64)
  np.add.at(wa, L, np.abs(p64))
  err = np.abs(sums.cpu().numpy() - ws) / wa
  assert err.max() <= 1e-5, err.max()


def test_kmeans_step_timing_hook(ex):
  """spx_kmeans_timing / spx_kmeans_times (bench.py's k-means kernel
  roofline): one (kernel, step) pair per fused step in call order, the kernel
  inside the step, nothing recorded while off, and the results unchanged."""
  import torch
  from spartan_amd import backend
  be = backend.get()
  N, D, K = 200_000, 128, 256
  P = torch.empty((N, D), dtype=torch.float32, device='cuda')
  be.fill(P, backend.FILL_UNIFORM, 0.0, 1.0, 5, (0, 0), (N, D))
  Cd = P[:K].to(torch.float64).contiguous()
  lab = torch.empty((N,), dtype=torch.int64, device='cuda')
  sums = torch.empty((K, D), dtype=torch.float64, device='cuda')
  cnt = torch.empty((K,), dtype=torch.int64, device='cuda')
  be.kmeans_step(P, Cd, lab, sums, cnt)
  s0, l0 = sums.clone(), lab.clone()
  be.kmeans_timing(True)
  try:
    for _ in range(3):
      be.kmeans_step(P, Cd, lab, sums, cnt)
    t = be.kmeans_times()
    assert len(t) == 3 and all(0.0 < a <= b for a, b in t), t
    assert be.kmeans_times() == []   # read once
  finally:
    be.kmeans_timing(False)
  be.kmeans_step(P, Cd, lab, sums, cnt)
  assert torch.equal(sums, s0) and torch.equal(lab, l0)
  with pytest.raises(RuntimeError):
    be.kmeans_times()                # timing is off


def test_kernel_events_log_the_timed_aot_calls(ex):
  """The timing contract bench.py reads (``kernel_events``): each timed
  ahead-of-time call logs one (name, start, end) triple in call order, the
  untimed ones (fill, copy_region, bincount) and an early return on an empty
  input log nothing, and with the list off nothing is logged or raised."""
  import math
  import torch
  from spartan_amd import backend
  be = backend.get()

  def dev(shape, dtype, fill=1):
    return torch.full(shape, fill, dtype=dtype, device='cuda')

  A, B, C = dev((4, 4), torch.float32), dev((4, 4), torch.float32), dev((4, 4), torch.float32)
  src_i, out_i = dev((8,), torch.int32), dev((8,), torch.int64)
  src_f, out_f = torch.arange(8, 0, -1, dtype=torch.float32, device='cuda'), dev((8,), torch.float32)
  A64, B64, C64 = dev((4, 4), torch.float64), dev((4, 4), torch.float64), dev((4, 4), torch.float64)
  filled = dev((8,), torch.float32, 0)
  dst, blk = dev((2, 2), torch.float32, 0), dev((2, 2), torch.float32)
  labels, counts = dev((8,), torch.int64), dev((2,), torch.int64, 0)
  empty = torch.empty((0,), dtype=torch.float32, device='cuda')
  be.kernel_events = []
  try:
    be.gemm(A, B, C)
    be.fill(filled, backend.FILL_CONST, 3.0, 0.0, 0, (0,), (8,))
    be.scan(src_i, out_i, (1, 8, 1))
    be.copy_region(dst, (0, 0), blk, (0, 0), (2, 2))
    be.sort(src_f, out_f, None, (1, 8, 1))
    be.sort(empty, torch.empty_like(empty), None, (0, 8, 1))
    be.bincount(labels, counts)
    be.syrk(A64, B64, C64)
    events = be.kernel_events
  finally:
    be.kernel_events = None
  torch.cuda.synchronize()
  assert [e[0] for e in events] == ['spx_gemm', 'spx_scan', 'spx_sort', 'spx_syrk']
  for e in events:
    assert len(e) == 3
    ms = e[1].elapsed_time(e[2])
    assert isinstance(ms, float) and math.isfinite(ms) and ms >= 0.0, e
  # the calls themselves ran: what each one wrote
  assert torch.equal(C, dev((4, 4), torch.float32, 4)) and torch.equal(filled, dev((8,), torch.float32, 3))
  assert out_i.tolist() == list(range(1, 9)) and out_f.tolist() == [float(v) for v in range(1, 9)]
  assert torch.equal(dst, blk) and counts.tolist() == [0, 8]
  assert torch.equal(C64, dev((4, 4), torch.float64, -3))
  be.gemm(A, B, C)
  assert be.kernel_events is None
