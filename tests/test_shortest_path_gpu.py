"""spx_apsp, the shortest_path expression layer and the Isomap driver on a real
MI355X, at the sizes where the blocked Floyd-Warshall kernels
can go wrong.  With b = apsp_plan(dtype): n = 1, 2 (one partial tile), b - 1, b,
b + 1 (a last block of one row), 2 b + 1 and 3 b -- three blocks are the fewest
at which k_apsp_rest has tiles on both sides of the pivot in both directions.
b + 4, and a leading dimension of b + 4 at n = b + 1, keep the rows of D 16-byte
aligned in float32 as well, so the 16-byte accesses run beside a partial block.

The yardstick is graph_ref.apsp_ref (scipy's Dijkstra on the float64 image of
the dtype-rounded weights).  Integer weights make every path sum exact in both
dtypes, so those cases are compared bit for bit; real weights are held to the
project's parity tolerances (1e-5 float32, 1e-12 float64), and the long chain
to the bound of a sum of h positive terms in any order, (h - 1) u relative.
"""
import ctypes

import numpy as np
import pytest

from graph_ref import apsp_ref, check_isomap, graph_data, isomap_model, swiss_roll

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
TOL = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-12}
UNIT = {np.dtype(np.float32): 2.0 ** -24, np.dtype(np.float64): 2.0 ** -53}
SEED = 0  # graph_data('int', n, ., 0): 1.6 % .. 11.2 % unreachable pairs at the block-sized n below (asserted)


def _b(dtype):
  from spartan_amd import backend
  return backend.apsp_plan(dtype)


def _dev(a):
  import torch
  return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _host(t):
  return t.cpu().numpy()


def _bits(a):
  return np.ascontiguousarray(a).view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _run(G, directed=True, unreachable=np.inf):
  """(D, info) on the host of one apsp call on the host matrix ``G``."""
  from spartan_amd import backend
  D, info = backend.get().apsp(_dev(G), directed, unreachable)
  return _host(D), int(_host(info)[0])


def _same(D, ref):
  """D (dtype) against the float64 yardstick: equal values, equal +inf pattern."""
  return np.array_equal(np.isinf(D), np.isinf(ref)) and np.array_equal(D.astype(np.float64), ref)


# --------------------------------------------------------------------- spx_apsp
@pytest.mark.parametrize('directed', [True, False])
@pytest.mark.parametrize('dtype', DTYPES)
def test_integer_weights_bit_for_bit(gpu_ctx, dtype, directed):
  b = _b(dtype)
  # b + 4: rows of D stay 16-byte aligned in float32 too, with a partial last block (vector path with a tail)
  for n in (1, 2, b - 1, b, b + 1, b + 4, 2 * b + 1, 3 * b):
    G = graph_data('int', n, dtype, SEED)
    ref = apsp_ref(G, directed)
    if directed and n >= b - 1:
      far = float(np.isinf(ref).mean())
      assert 0 < far <= 0.2, (n, far)  # some pairs without a path, most with one
    D, info = _run(G, directed)
    what = 'apsp int n=%d %s directed=%s' % (n, np.dtype(dtype), directed)
    assert info == 0, what
    assert D.dtype == np.dtype(dtype) and D.shape == (n, n), what
    assert _same(D, ref), '%s: %d entries differ' % (what, int((D.astype(np.float64) != ref).sum()))


@pytest.mark.parametrize('dtype', DTYPES)
def test_chain_crosses_every_block(gpu_ctx, dtype):
  """0 - 1 - ... - (n - 1): the longest path has n - 1 hops and every pivot
  block lies on it."""
  n = 3 * _b(dtype)
  hops = np.abs(np.arange(n)[:, None] - np.arange(n)[None, :]).astype(np.float64)
  D, info = _run(graph_data('chain', n, dtype, weight=1.0), False)
  assert info == 0 and _same(D, hops)  # exact
  D, info = _run(graph_data('chain', n, dtype, weight=1.0), True)  # directed: nothing leads back
  assert info == 0 and _same(D, np.where(np.arange(n)[:, None] <= np.arange(n)[None, :], hops, np.inf))
  G = graph_data('chain', n, dtype, weight=0.1)
  ref = apsp_ref(G, False)
  D, info = _run(G, False)
  err = np.abs(D.astype(np.float64) - ref)
  lim = np.maximum(hops - 1, 0) * UNIT[np.dtype(dtype)] * ref * 1.01 + UNIT[np.dtype(dtype)] * ref  # + the final rounding
  print('chain 0.1 %s: worst error / bound %.3g' % (np.dtype(dtype), float((err / np.where(lim > 0, lim, 1)).max())))
  assert info == 0 and np.all(err <= lim)


@pytest.mark.parametrize('dtype', DTYPES)
def test_neighbour_graph_real_weights(gpu_ctx, dtype):
  b = _b(dtype)
  for n in (2 * b + 1, 3 * b):
    G = graph_data('knn', n, dtype, SEED)
    ref = apsp_ref(G, False)
    assert np.all(np.isfinite(ref)), n  # connected
    D, info = _run(G, False)
    assert info == 0 and np.all(np.isfinite(D))
    rel = np.abs(D.astype(np.float64) - ref) / np.where(ref > 0, ref, 1)
    print('apsp knn n=%d %s: worst relative error %.3g' % (n, np.dtype(dtype), float(rel.max())))
    assert np.all(np.abs(D.astype(np.float64) - ref) <= TOL[np.dtype(dtype)] * ref)


@pytest.mark.parametrize('dtype', DTYPES)
def test_forms(gpu_ctx, dtype):
  """Padded leading dimensions through the ABI, the two spellings of "no edge",
  the ignored diagonal, ``unreachable``, bad weights and the empty graph."""
  import torch
  from spartan_amd import backend
  be = backend.get()
  n = _b(dtype) + 1
  G = graph_data('int', n, dtype, SEED)
  for directed in (True, False):
    want, info = _run(G, directed)
    assert info == 0 and np.isinf(want).any() == directed
    # padded G and D through the ABI; the sentinels survive
    gbuf = np.full((n, n + 3), -7.0, dtype)  # a negative pad: reading it would set info
    gbuf[:, :n] = G
    tg = _dev(gbuf)
    # ldd = n + 5: rows of D that are not 16-byte aligned in float32 (element accesses).  ldd = n + 3 = b + 4:
    # aligned rows in both dtypes, so the 16-byte accesses run and the last vector of a row would cross column n
    for ldd in (n + 5, n + 3):
      td = _dev(np.full((n, ldd), 77.0, dtype))
      ti = torch.full((1,), 55, dtype=torch.int32, device='cuda')
      rc = be.lib.spx_apsp(backend.spx_dtype(dtype), int(directed), n, ctypes.c_void_p(tg.data_ptr()), n + 3,
                           ctypes.c_void_p(td.data_ptr()), ldd, float('inf'), ctypes.c_void_p(ti.data_ptr()),
                           be.stream())
      assert rc == 0
      hd = _host(td)
      assert int(_host(ti)[0]) == 0
      assert np.array_equal(_bits(hd[:, :n]), _bits(want)) and np.all(hd[:, n:] == 77.0), ldd
      assert np.array_equal(_bits(_host(tg)), _bits(gbuf))  # G and its pads untouched
    # the strided view through the backend
    D2, i2 = be.apsp(tg[:, :n], directed)
    assert np.array_equal(_bits(_host(D2)), _bits(want)) and int(_host(i2)[0]) == 0
    # +inf for "no edge", junk on the diagonal
    H = G.copy()
    H[H == 0] = np.inf
    H[np.arange(n), np.arange(n)] = np.where(np.arange(n) % 2, 5.0, np.inf)
    D3, i3 = _run(H, directed)
    assert i3 == 0 and np.array_equal(_bits(D3), _bits(want))
    # unreachable = 0.0 rewrites exactly the +inf entries
    D4, i4 = _run(G, directed, 0.0)
    assert i4 == 0 and np.array_equal(_bits(D4), _bits(np.where(np.isinf(want), 0, want).astype(dtype)))
    # determinism
    again, _ = _run(G, directed)
    assert np.array_equal(_bits(again), _bits(want))
  for bad in (-1.0, float('nan'), -np.inf):
    B = G.copy()
    B[n - 1, 3] = bad
    _, info = _run(B)  # returns; D is unspecified
    assert info == -1, bad
  E, info = _run(graph_data('empty', n, dtype), True, 9.0)
  assert info == 0 and np.array_equal(E, np.where(np.eye(n, dtype=bool), 0, 9).astype(dtype))


# ------------------------------------------------------------- expression layer
@pytest.mark.parametrize('dtype', DTYPES)
def test_expression_layer_dense_and_sparse(gpu_ctx, gpu_workers, dtype):
  import scipy.sparse as sp
  from spartan_amd import expr
  gpu_workers(3)
  n = _b(dtype) + 1
  G = graph_data('int', n, dtype, SEED)
  for directed in (True, False):
    ref = apsp_ref(G, directed)
    dense = expr.shortest_path(expr.from_numpy(G, tile_hint=(24, 40)), directed=directed)
    assert dense.shape == (n, n) and dense.dtype == np.dtype(dtype)
    assert _same(dense.glom(), ref)
    sparse = expr.shortest_path(expr.from_numpy(sp.csr_matrix(G), tile_hint=(24, n)), directed=directed).force()
    assert sorted(e.ul[0] for e in sparse.tiles) == list(range(0, n, 24))  # row slabs at the input's cuts
    assert _same(sparse.glom(), ref)
  bad = G.copy()
  bad[1, 2] = -3
  with pytest.raises(ValueError, match='negative or NaN edge weight'):
    expr.shortest_path(expr.from_numpy(bad, tile_hint=(24, 40))).force()


def test_isomap_on_the_device(gpu_ctx):
  from spartan_amd.examples.isomap import Isomap
  X = swiss_roll(150, seed=0)
  tol = 1e-8
  model = isomap_model(X, 8, 2)
  iso = Isomap(n_neighbors=8, n_components=2, tol=tol).fit(X)
  assert 0 < iso.n_iter_ < 200
  check_isomap(model, iso, tol, 'isomap gpu')
