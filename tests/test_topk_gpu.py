"""GPU parity of topk / argtopk and the fused nearest-neighbour search:
``HipBackend.topk`` (spx_topk: the LDS path and the radix-select path,
contiguous and strided lines) and ``HipBackend.knn`` (spx_knn) against the
NumPy oracle of tests/topk_ref.py, then ``spartan_amd.topk`` / ``argtopk`` and
``NearestNeighbors`` over tile layouts.

Everything is exact: positions equal the stable order's first k, values carry
the selected input elements' bits (NaNs match NaNs), the nearest-neighbour
sums equal the oracle's fp64 sums bit for bit.

Cases are capped at 2^21 elements as in tests/test_sort_gpu.py.  With inner =
65 that drops (n, inner, outer) = (chunk - 1 | chunk | chunk + 1, 65, 5) and (2
chunk + 1031, 65, 1 | 5); every other (n, inner, outer) runs, and no data kind
or dtype is dropped.
"""
import numpy as np
import pytest

from topk_ref import knn_data, knn_ref, order_ref, same_bits, sort_data, topk_ref

pytestmark = pytest.mark.gpu

MAX_ELEMS = 1 << 21
DTYPES = [np.bool_, np.int32, np.int64, np.float32, np.float64]
KINDS = ['uniform', 'dup7', 'equal', 'asc', 'desc', 'extremes']
INNERS = [1, 3, 65]
OUTERS = [1, 5]


def _consts():
  from spartan_amd import backend
  L = backend.SORT_LDS_MAX
  return L, backend.topk_plan(1, L + 1, 1, np.float32)[2], backend.TOPK_K_MAX


def _ns():
  L, C, _ = _consts()
  return [1, 2, 63, 64, 65, L - 1, L, L + 1, 3 * L + 17, C - 1, C, C + 1, 2 * C + 1031]


N_CASES = 13  # len(_ns()), fixed so that collection needs no library


def _geoms(n, inner):
  return [(o, n, inner) for o in OUTERS if o * n * inner <= MAX_ELEMS]


def _ks(n):
  kmax = _consts()[2]
  return sorted({k for k in (1, 2, 7, 64, min(n, kmax)) if k <= n})


def _dev(a):
  import torch
  return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _empty(shape, dt):
  import torch
  from spartan_amd import backend
  return torch.empty(shape, dtype=backend.torch_dtype(dt), device='cuda')


def _want(x, order, k):
  idx = order[:, :k, :]
  return np.take_along_axis(x, idx, 1), idx


def _run_forms(be, src, x, k, largest, want_v, want_i, payload=None):
  """The three call forms, a repeat and the payload form of one (input, k, direction)."""
  import torch
  o, n, i = x.shape
  shape = (o, k, i)
  vals, idx = _empty(shape, x.dtype), _empty(shape, np.int64)
  both_v, both_i = _empty(shape, x.dtype), _empty(shape, np.int64)
  be.topk(src, None, vals, None, (o, n, i), k, largest)
  be.topk(src, None, None, idx, (o, n, i), k, largest)
  be.topk(src, None, both_v, both_i, (o, n, i), k, largest)
  again_v, again_i = _empty(shape, x.dtype), _empty(shape, np.int64)
  be.topk(src, None, again_v, again_i, (o, n, i), k, largest)
  assert torch.equal(both_i, again_i)
  assert torch.equal(both_v.view(torch.uint8), again_v.view(torch.uint8))  # the same bits
  msg = '%s %s k=%d largest=%s' % (x.shape, x.dtype, k, largest)
  for t in (idx, both_i):
    np.testing.assert_array_equal(t.cpu().numpy(), want_i, err_msg=msg)
  for t in (vals, both_v):
    assert same_bits(t.cpu().numpy(), want_v), msg
  if payload is not None:
    pay_v, pay_i = _empty(shape, x.dtype), _empty(shape, np.int64)
    be.topk(src, payload[0], pay_v, pay_i, (o, n, i), k, largest)
    np.testing.assert_array_equal(pay_i.cpu().numpy(), np.take_along_axis(payload[1], want_i, 1), err_msg=msg)
    assert same_bits(pay_v.cpu().numpy(), want_v), msg


def _run_one(be, src, x, k, largest, want_v, want_i):
  shape = (x.shape[0], k, x.shape[2])
  v, i = _empty(shape, x.dtype), _empty(shape, np.int64)
  be.topk(src, None, v, i, x.shape, k, largest)
  msg = '%s %s k=%d largest=%s' % (x.shape, x.dtype, k, largest)
  np.testing.assert_array_equal(i.cpu().numpy(), want_i, err_msg=msg)
  assert same_bits(v.cpu().numpy(), want_v), msg


@pytest.mark.parametrize('inner', INNERS)
@pytest.mark.parametrize('ni', range(N_CASES))
def test_backend_topk_geometries(gpu_workers, ni, inner):
  """Every geometry x dtype x k x direction.  The data kind rotates with the
  case so each kind meets each path, and 'extremes' (NaN, +-0, INT_MIN) also
  meets every case of at most 2^18 elements; each (input, direction) runs
  every k, one of them in all call forms."""
  gpu_workers(1)
  import torch
  from spartan_amd import backend
  be = backend.get()
  assert len(_ns()) == N_CASES
  n = _ns()[ni]
  r = np.random.RandomState(ni * 7 + inner)
  for gi, (o, n, i) in enumerate(_geoms(n, inner)):
    for di, dt in enumerate(DTYPES):
      kinds = [KINDS[(ni + di + gi) % len(KINDS)]]
      if o * n * i <= 1 << 18:  # the large cases meet 'extremes' through the rotation alone
        kinds.append('extremes')
      for kind in kinds:
        x = sort_data((o, n, i), dt, kind, 1000 * ni + 10 * inner + di)
        src = _dev(x)
        pay = r.randint(-2 ** 62, 2 ** 62, x.shape, dtype=np.int64)
        for largest in (False, True):
          order = order_ref(x, 1, largest)
          ks = _ks(n)
          full = ks[(ni + di) % len(ks)]
          for k in ks:
            want_v, want_i = _want(x, order, k)
            if k == full:
              _run_forms(be, src, x, k, largest, want_v, want_i, (_dev(pay), pay))
            else:
              _run_one(be, src, x, k, largest, want_v, want_i)
        assert torch.equal(src.cpu().view(torch.uint8), torch.as_tensor(x).view(torch.uint8))  # input untouched


@pytest.mark.parametrize('dt', DTYPES)
def test_backend_topk_every_kind_on_both_paths(gpu_workers, dt):
  gpu_workers(1)
  from spartan_amd import backend
  be = backend.get()
  L, C, _ = _consts()
  for (o, n, i) in ((3, 777, 1), (2, 300, 5), (2, C + L + 77, 1), (1, L + 9, 3)):
    for ki, kind in enumerate(KINDS):
      x = sort_data((o, n, i), dt, kind, 50 + ki)
      src = _dev(x)
      for largest in (False, True):
        order = order_ref(x, 1, largest)
        for k in (1, 33, min(n, 1500)):
          _run_one(be, src, x, k, largest, *_want(x, order, k))


@pytest.mark.parametrize('dt', DTYPES)
def test_backend_topk_each_radix_digit_alone(gpu_workers, dt):
  """Keys that differ in one 8-bit digit only: a select pass that narrowed
  nothing, or the wrong way, shows here."""
  gpu_workers(1)
  from spartan_amd import backend
  from sort_ref import key_bits
  be = backend.get()
  L, C, _ = _consts()
  for digit in range(key_bits(dt) // 8):
    for (o, n, i) in ((2, C + 3 * L + 5, 1), (1, L + 1, 3)):
      x = sort_data((o, n, i), dt, 'digit', 7 + digit, digit=digit)
      src = _dev(x)
      for largest in (False, True):
        order = order_ref(x, 1, largest)
        for k in (5, 300):
          _run_one(be, src, x, k, largest, *_want(x, order, k))


def test_both_paths_run_for_both_layouts(gpu_ctx):
  from spartan_amd import backend
  seen = set()
  for n in _ns():
    for inner in INNERS:
      for (o, n_, i) in _geoms(n, inner):
        path, passes, _c = backend.topk_plan(o, n_, i, np.float32)
        assert (path == 'lds') == (n_ <= backend.SORT_LDS_MAX) and (passes > 0) == (path == 'select')
        seen.add((path, 'row' if i == 1 else 'col'))
  assert seen == {('lds', 'row'), ('select', 'row'), ('lds', 'col'), ('select', 'col')}, seen
  L, C, K = _consts()
  assert _ns()[-1] > 2 * C and _ns()[-1] % C != 0 and K == L  # three chunks, the last one ragged


def test_backend_topk_argument_checks(gpu_workers):
  gpu_workers(1)
  from spartan_amd import backend
  be = backend.get()
  x = _dev(np.arange(12, dtype=np.float32))
  ov, oi = _empty((3,), np.float32), _empty((3,), np.int64)
  with pytest.raises(ValueError):
    be.topk(x, None, None, None, (1, 12, 1), 3)
  with pytest.raises(ValueError):
    be.topk(x, None, _empty((3,), np.float64), None, (1, 12, 1), 3)
  with pytest.raises(ValueError):
    be.topk(x, None, None, _empty((3,), np.int32), (1, 12, 1), 3)
  with pytest.raises(ValueError):
    be.topk(x, None, _empty((4,), np.float32), None, (1, 12, 1), 3)
  with pytest.raises(ValueError):
    be.topk(x, None, ov, oi, (1, 13, 1), 3)
  for k in (0, 13):
    with pytest.raises(ValueError):
      be.topk(x, None, ov, oi, (1, 12, 1), k)
  with pytest.raises(ValueError):
    be.topk(x, _empty((11,), np.int64), ov, oi, (1, 12, 1), 3)
  with pytest.raises(ValueError):
    be.topk(x.reshape(3, 4).t(), None, ov, oi, (1, 12, 1), 3)
  big = _dev(np.zeros(3 * backend.TOPK_K_MAX, np.float32))
  with pytest.raises(ValueError, match='TOPK_K_MAX'):
    be.topk(big, None, None, _empty((backend.TOPK_K_MAX + 1,), np.int64), (1, big.numel(), 1),
            backend.TOPK_K_MAX + 1)


# ------------------------------------------------------ nearest neighbours
def _knn_consts():
  from spartan_amd import backend
  return backend.knn_plan(1, 1, 1, 1)[1], backend.KNN_K_MAX


def _knn_case(be, kind, Q, N, D, k, dt, seed, pad=0, base=0):
  import torch
  X, q = knn_data(kind, N, Q, D, dt, seed)
  want_s, want_i = knn_ref(X, q, k)
  if pad:
    buf = _empty((N, D + pad), dt)
    buf.fill_(float('nan'))  # a kernel that read past D would show
    buf[:, :D] = _dev(X)
    pts = buf[:, :D]
    assert pts.stride(0) == D + pad and not pts.is_contiguous()
  else:
    pts = _dev(X)
  qd = _dev(q.astype(np.float64))
  out_s, out_i = _empty((Q, k), np.float64), _empty((Q, k), np.int64)
  be.knn(pts, qd, k, base, out_s, out_i)
  again_s, again_i = _empty((Q, k), np.float64), _empty((Q, k), np.int64)
  be.knn(pts, qd, k, base, again_s, again_i)
  assert torch.equal(out_i, again_i) and torch.equal(out_s.view(torch.uint8), again_s.view(torch.uint8))
  msg = '%s Q=%d N=%d D=%d k=%d %s pad=%d base=%d' % (kind, Q, N, D, k, np.dtype(dt), pad, base)
  np.testing.assert_array_equal(out_i.cpu().numpy(), want_i + base, err_msg=msg)
  assert same_bits(out_s.cpu().numpy(), want_s), msg


KNN_KINDS = ['grid', 'uniform', 'dup', 'far', 'nonfinite']
BASE = dict(Q=65, N=4097, D=17, k=5)


@pytest.mark.parametrize('dt', [np.float32, np.float64])
@pytest.mark.parametrize('kind', KNN_KINDS)
def test_backend_knn_kinds(gpu_workers, kind, dt):
  """Every data kind and both dtypes at the base case, contiguous and with ldp > D."""
  gpu_workers(1)
  from spartan_amd import backend
  be = backend.get()
  _knn_case(be, kind, dt=dt, seed=3, **BASE)
  _knn_case(be, kind, dt=dt, seed=4, pad=3, base=10 ** 12 + 7, **BASE)


@pytest.mark.parametrize('param', ['Q', 'N', 'D', 'k'])
def test_backend_knn_every_value_of_each_parameter(gpu_workers, param):
  """Each parameter over all its values against the fixed base case (the
  cross product taken sparsely); the data kind and dtype rotate."""
  gpu_workers(1)
  from spartan_amd import backend
  be = backend.get()
  chunk, kmax = _knn_consts()
  values = {'Q': [1, 63, 65], 'N': [None, 63, 64, 65, 4097, chunk - 1, chunk + 1, 2 * chunk + 77],
            'D': [1, 15, 16, 17, 40], 'k': [1, 5, 64, kmax]}[param]
  for vi, v in enumerate(values):
    case = dict(BASE)
    case[param] = v
    if param == 'N':
      for k in (5, 64):  # N = k (every point selected) and the short N
        c = dict(case, k=k)
        c['N'] = k if v is None else v
        if c['k'] <= c['N']:
          _knn_case(be, KNN_KINDS[(vi + k) % 5], dt=[np.float32, np.float64][vi % 2], seed=20 + vi, **c)
    else:
      for j in range(2):
        _knn_case(be, KNN_KINDS[(vi + 2 * j) % 5], dt=[np.float32, np.float64][(vi + j) % 2], seed=40 + vi, **case)
  if param == 'k':  # the largest k over several ranges, ties everywhere
    _knn_case(be, 'grid', Q=63, N=2 * chunk + 77, D=3, k=kmax, dt=np.float32, seed=9, base=5)
    assert backend.knn_plan(63, 2 * chunk + 77, 3, kmax)[0] == 3 and backend.knn_plan(65, 4097, 17, 5)[0] > 1
    # so many ranges that their lists are longer than one LDS sort: the select path combines them
    assert backend.knn_plan(3, 17 * chunk + 5, 2, kmax)[0] * kmax > backend.SORT_LDS_MAX
    _knn_case(be, 'dup', Q=3, N=17 * chunk + 5, D=2, k=kmax, dt=np.float64, seed=10)


def test_backend_knn_argument_checks(gpu_workers):
  gpu_workers(1)
  from spartan_amd import backend
  be = backend.get()
  X, q = _dev(np.zeros((20, 3), np.float32)), _dev(np.zeros((4, 3)))
  s, i = _empty((4, 5), np.float64), _empty((4, 5), np.int64)
  with pytest.raises(ValueError):
    be.knn(X, _dev(np.zeros((4, 3), np.float32)), 5, 0, s, i)
  with pytest.raises(ValueError):
    be.knn(X, _dev(np.zeros((4, 2))), 5, 0, s, i)
  with pytest.raises(ValueError):
    be.knn(X.to(dtype=__import__('torch').int32), q, 5, 0, s, i)
  with pytest.raises(ValueError):
    be.knn(X, q, 5, 0, _empty((4, 4), np.float64), i)
  with pytest.raises(ValueError):
    be.knn(X, q, 5, 0, s, _empty((4, 5), np.int32))
  for k in (0, 21):
    with pytest.raises(ValueError):
      be.knn(X, q, k, 0, s, i)
  with pytest.raises(ValueError, match='KNN_K_MAX'):
    n = backend.KNN_K_MAX + 1
    be.knn(_dev(np.zeros((2 * n, 3), np.float32)), q, n, 0, _empty((4, n), np.float64), _empty((4, n), np.int64))


# ------------------------------------------------------- expression level
def _expr_shapes():
  L, C, _ = _consts()
  return [((257, 4099), (64, 1000)), ((70001,), (9973,)), ((3, 50, 130), (2, 17, 48)), ((C + L + 3,), (L + 5,))]


_REF = {}


def _ref(si, kind, axis, largest):
  """(input, full stable order) of one case, computed once."""
  key = (si, kind, axis, largest)
  if key not in _REF:
    shape = _expr_shapes()[si][0]
    dt, dk = {'int64': (np.int64, 'uniform'), 'f32_dup': (np.float32, 'dup7'), 'f64_nan': (np.float64, 'extremes')}[kind]
    a = sort_data((1, int(np.prod(shape)), 1), dt, dk, 31 + si).reshape(shape)
    _REF[key] = (a, order_ref(a, axis, largest))
  return _REF[key]


@pytest.mark.parametrize('kind', ['int64', 'f32_dup', 'f64_nan'])
@pytest.mark.parametrize('si', [0, 1, 2, 3])
@pytest.mark.parametrize('W', [1, 3])
def test_expr_topk(gpu_workers, W, si, kind):
  gpu_workers(W)
  from spartan_amd import expr
  shape, split = _expr_shapes()[si]
  for hint in (None, split):
    for axis in range(len(shape)):
      for largest in (False, True):
        a, order = _ref(si, kind, axis, largest)
        k = min(a.shape[axis], 9 if largest else 40)
        want_i = np.take(order, np.arange(k), axis=axis)
        want_v = np.take_along_axis(a, want_i, axis)
        x = expr.from_numpy(a, tile_hint=hint)
        e, g = expr.topk(x, k, axis, largest), expr.argtopk(x, k, axis, largest)
        got_v, got_i = e.glom(), g.glom()
        assert got_v.dtype == a.dtype == e.dtype and got_i.dtype == np.int64 == g.dtype
        assert got_v.shape == want_v.shape == e.shape == g.shape == got_i.shape
        msg = '%s %s %s' % (hint, axis, largest)
        np.testing.assert_array_equal(got_i, want_i, err_msg=msg)
        assert same_bits(got_v, want_v), msg


def test_expr_topk_of_lazy_input_and_view(gpu_workers):
  gpu_workers(3)
  from spartan_amd import expr
  a = sort_data((1, 130 * 257, 1), np.int32, 'uniform', 3).reshape(130, 257) % 1000
  x = expr.from_numpy(a, tile_hint=(40, 100))
  np.testing.assert_array_equal((expr.topk(x * 2, 11, axis=0) + 1).optimized().glom(), topk_ref(a * 2, 11, 0)[0] + 1)
  v = a[5:120, 3:250].T
  np.testing.assert_array_equal(expr.argtopk(x[5:120, 3:250].T, 9, axis=1, largest=True).glom(),
                                topk_ref(v, 9, 1, True)[1])
  np.testing.assert_array_equal(expr.topk(expr.as_array(a) * 2, 4, axis=1).glom(), topk_ref(a * 2, 4, 1)[0])


@pytest.mark.parametrize('dt', [np.float32, np.float64])
@pytest.mark.parametrize('W', [1, 3])
def test_nearest_neighbors(gpu_workers, W, dt):
  gpu_workers(W)
  from spartan_amd import expr
  from spartan_amd.examples.neighbors import NearestNeighbors
  # the reference test's shape, then row tiles, row + column tiles and blocks shorter than k
  cases = [('uniform', 20000, 2 * W, 2 * W, 10, None), ('far', 5000, 33, 7, 10, (1300, 7)),
           ('grid', 3000, 9, 5, 64, (700, 3)), ('nonfinite', 900, 5, 6, 20, (7, 6))]
  for kind, N, Q, D, k, hint in cases:
    X, q = knn_data(kind, N, Q, D, dt, 17)
    s, want_i = knn_ref(X, q, k)
    nn = NearestNeighbors(n_neighbors=k).fit(expr.from_numpy(X, tile_hint=hint))
    dist, ind = nn.kneighbors(q)
    assert dist.dtype == np.dtype(dt) and ind.dtype == np.int64 and dist.shape == ind.shape == (Q, k)
    msg = '%s %s' % (kind, hint)
    np.testing.assert_array_equal(ind, want_i, err_msg=msg)
    assert same_bits(dist, np.sqrt(s).astype(dt)), msg
