"""``spartan_amd.eigh`` host logic (no GPU): every route of the expression layer
over tile layouts and worker counts, laziness, validation, LinAlgError, two
gloo ranks, the plan / no-launch answers of spx_syevj, the NumPy model that is
half of the yardstick, and the lanczos / svds drivers.

The expression layer runs here over the CPU test double with a scipy ``syevj``
(eigh_ref.EighFakeBackend); the kernel itself is tested on the GPU in
tests/test_eigh_gpu.py.
"""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(ROOT, 'spartan_amd', 'libspx.so')

needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason='libspx.so not built')

N2 = 10
HINTS2 = [(10, 10), (4, 10), (10, 3), (4, 3)]
SHAPE3 = (7, 6, 6)
HINTS3 = [(7, 6, 6), (2, 6, 6), (3, 4, 6), (2, 6, 2)]  # one tile; batch slabs; two layouts cut inside the matrices
SLAB_HINTS = [(7, 6, 6), (2, 6, 6)]


@pytest.fixture
def eigh_ctx(host_ctx):
  """host_ctx with the eigh-capable test double installed."""
  from spartan_amd import backend
  from eigh_ref import EighFakeBackend

  def make(num_workers=1):
    host_ctx(num_workers)
    be = EighFakeBackend()
    backend.set_backend(be)
    return be
  return make


@pytest.fixture
def gathers(monkeypatch):
  """Counts the ``gather_regions`` exchanges."""
  from spartan_amd.array import distarray
  calls = []
  real = distarray.gather_regions

  def counted(array, requests):
    calls.append(len(requests))
    return real(array, requests)
  monkeypatch.setattr(distarray, 'gather_regions', counted)
  return calls


def _replicated(a):
  import torch
  from spartan_amd import expr
  from spartan_amd.array import distarray
  return expr.lazify(distarray.ReplicatedArray(torch.as_tensor(a.copy())))


def _stack(dtype, seed=0):
  """(7, 6, 6): one matrix of seven different kinds."""
  from eigh_ref import eigh_data
  kinds = ('gauss', 'tridiag', 'posdef', 'diag', 'zero', 'cluster', 'exchange')
  return np.stack([eigh_data(k, SHAPE3[1], dtype, seed)[0] for k in kinds])


def _check(A, w, V, what):
  """The test double is LAPACK: its ratios stay within the yardstick's margin."""
  from eigh_ref import FACTOR, check_form, eigh_ratios, yardstick
  n = A.shape[0]
  assert w.dtype == A.dtype and V.dtype == A.dtype and w.shape == (n,) and V.shape == (n, n)
  check_form(w, V)
  yard = yardstick(A.dtype, n)
  res, orth, _ = eigh_ratios(A, w, V)
  print('%s: res %.3g u (yardstick %.3g), orth %.3g u (yardstick %.3g)' % (what, res, yard[0], orth, yard[1]))
  assert res <= FACTOR * yard[0] and orth <= FACTOR * yard[1], what


# ------------------------------------------------------------- expr layer
@needs_lib
@pytest.mark.parametrize('W', [1, 3])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_eigh_2d_every_route(eigh_ctx, gathers, W, dtype):
  be = eigh_ctx(W)
  from spartan_amd import expr
  from spartan_amd.array import distarray
  from eigh_ref import eigh_data, same_bits
  A, _ = eigh_data('gauss', N2, dtype)
  first = None
  for hint in HINTS2 + ['replicated', 'host']:
    if hint == 'replicated':
      x = _replicated(A)
    elif hint == 'host':
      x = A
    else:
      x = expr.lazify(expr.from_numpy(A, tile_hint=hint).force())
    del be.calls[:]
    del gathers[:]
    we, ve = expr.eigh(x)
    wa, va = we.force(), ve.force()
    assert isinstance(wa, distarray.ReplicatedArray) and isinstance(va, distarray.ReplicatedArray), hint
    assert be.calls.count('syevj') == 1, hint
    assert len(gathers) == (0 if hint == 'replicated' else 1), hint  # ONE exchange of the whole matrix
    w, V = wa.glom(), va.glom()
    _check(A, w, V, 'eigh 2-d %s W=%d %s' % (hint, W, np.dtype(dtype)))
    if first is None:
      first = (w, V)
    assert same_bits(w, first[0]) and same_bits(V, first[1]), hint  # the same bits for every layout
  # the upper triangle, and eigvalsh
  wu = expr.eigvalsh(expr.from_numpy(A, tile_hint=(4, 3)), UPLO='U').glom()
  assert same_bits(wu, first[0])
  B = A.copy()
  B[np.triu_indices(N2, 1)] = np.nan  # the triangle that is not read
  assert same_bits(expr.eigh(B)[1].glom(), first[1])
  assert same_bits(expr.eigh(B.T, UPLO='U')[1].glom(), first[1])


@needs_lib
@pytest.mark.parametrize('W', [1, 3])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_eigh_3d_every_route(eigh_ctx, gathers, W, dtype):
  be = eigh_ctx(W)
  from spartan_amd import expr
  from spartan_amd.array import distarray
  from eigh_ref import same_bits
  A = _stack(dtype)
  first = None
  for hint in HINTS3 + ['replicated']:
    if hint == 'replicated':
      x = distarray.ReplicatedArray(__import__('torch').as_tensor(A.copy()))
    else:
      x = expr.from_numpy(A, tile_hint=hint).force()
    del be.calls[:]
    del gathers[:]
    we, ve = expr.eigh(expr.lazify(x))
    assert we.shape == SHAPE3[:2] and ve.shape == SHAPE3
    wa, va = we.force(), ve.force()
    if hint == 'replicated':
      assert isinstance(wa, distarray.ReplicatedArray) and isinstance(va, distarray.ReplicatedArray)
      assert be.calls.count('syevj') == 1 and not gathers
    else:
      assert va.tiles == x.tiles, hint  # V has A's tiling
      cuts = sorted({(e.ul[0], e.lr[0]) for e in x.tiles})
      assert sorted((e.ul[0], e.lr[0]) for e in wa.tiles) == cuts, hint  # w is cut along axis 0 at the same places
      assert all(e.ul[1] == 0 and e.lr[1] == SHAPE3[1] for e in wa.tiles)
      if hint in SLAB_HINTS:
        assert be.calls.count('syevj') == len(x.tiles) and not gathers, hint  # one call per tile, no exchange
        for e, wk in x.tiles.items():  # on the same workers
          assert [k for t, k in wa.tiles.items() if t.ul[0] == e.ul[0]] == [wk]
      else:
        assert be.calls.count('syevj') == len(cuts) and len(gathers) == 1, hint  # one call per slab, one exchange
    w, V = wa.glom(), va.glom()
    assert w.shape == SHAPE3[:2] and V.shape == SHAPE3
    for b in range(SHAPE3[0]):
      _check(A[b], w[b], V[b], 'eigh 3-d %s W=%d matrix %d' % (hint, W, b))
    if first is None:
      first = (w, V)
    assert same_bits(w, first[0]) and same_bits(V, first[1]), hint


@needs_lib
def test_lazy_shape_dtype_and_one_call(eigh_ctx):
  be = eigh_ctx(3)
  from spartan_amd import expr
  from eigh_ref import eigh_data
  A, _ = eigh_data('gauss', N2, np.float64, 3)
  we, ve = expr.eigh(expr.from_numpy(A, tile_hint=(4, 3)))
  assert isinstance(we, expr.Expr) and isinstance(ve, expr.Expr)
  assert we.shape == (N2,) and ve.shape == (N2, N2) and we.dtype == np.float64 and ve.dtype == np.float64
  prod = expr.dot(ve * we, expr.transpose(ve))  # V diag(w) V^T, still lazy
  assert 'syevj' not in be.calls
  w = we.glom()
  assert be.calls.count('syevj') == 1
  V = ve.glom()
  assert be.calls.count('syevj') == 1  # the pair shares one evaluation
  np.testing.assert_allclose(prod.glom(), A, atol=1e-12)
  assert be.calls.count('syevj') == 1
  np.testing.assert_allclose(w, np.linalg.eigvalsh(A), atol=1e-12)
  np.testing.assert_allclose(np.abs(V), np.abs(np.linalg.eigh(A)[1]), atol=1e-10)


@needs_lib
def test_validation_errors(eigh_ctx):
  eigh_ctx(1)
  from spartan_amd import backend, expr
  for bad in (np.ones(4), np.ones((3, 4)), np.ones((2, 3, 4)), np.ones((2, 2, 3, 3))):
    with pytest.raises(ValueError, match='square'):
      expr.eigh(bad)
  with pytest.raises(TypeError, match='float32 / float64'):
    expr.eigh(np.ones((4, 4), np.int64))
  with pytest.raises(ValueError, match='UPLO'):
    expr.eigh(np.ones((4, 4)), UPLO='X')
  for dt in (np.float32, np.float64):
    nmax, _ = backend.syevj_plan(dt)
    with pytest.raises(NotImplementedError, match='limit of %d' % nmax):
      expr.eigh(np.ones((nmax + 1, nmax + 1), dt))
    with pytest.raises(NotImplementedError, match='limit of %d' % nmax):
      expr.eigvalsh(np.ones((2, nmax + 1, nmax + 1), dt))
    expr.eigh(np.ones((nmax, nmax), dt))  # the limit itself is accepted
  sp = expr.sparse_diagonal((6, 6), dtype=np.float64)
  with pytest.raises(TypeError, match='sparse'):
    expr.eigh(sp)[0].force()


@needs_lib
@pytest.mark.parametrize('W', [1, 3])
def test_linalg_error(eigh_ctx, W):
  eigh_ctx(W)
  from spartan_amd import expr
  from eigh_ref import eigh_data
  A, _ = eigh_data('gauss', N2, np.float64)
  A[7, 2] = np.nan
  for hint in HINTS2:
    with pytest.raises(np.linalg.LinAlgError, match='Eigenvalues did not converge'):
      expr.eigh(expr.from_numpy(A, tile_hint=hint))[0].force()
  with pytest.raises(np.linalg.LinAlgError, match='Eigenvalues did not converge'):
    expr.eigvalsh(_replicated(A)).force()
  A[7, 2] = A[2, 7]
  A[2, 7] = np.inf  # the upper triangle is not read ...
  expr.eigh(A)[0].force()
  with pytest.raises(np.linalg.LinAlgError):  # ... unless it is asked for
    expr.eigh(A, UPLO='U')[0].force()
  S = _stack(np.float64)
  S[5, 3, 1] = np.nan
  for hint in HINTS3:
    with pytest.raises(np.linalg.LinAlgError, match='Eigenvalues did not converge'):
      expr.eigh(expr.from_numpy(S, tile_hint=hint))[1].force()


# --------------------------------------------------------------- gloo ranks
def _free_port():
  s = socket.socket()
  s.bind(('127.0.0.1', 0))
  p = s.getsockname()[1]
  s.close()
  return p


def _gloo_body(rank, world, port, W, q):
  try:
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank), SPARTAN_SPMD_GUARD='strict',
                      SPARTAN_NCCL_TIMEOUT='240')
    from spartan_amd import backend, runtime, expr
    from spartan_amd.array import distarray
    from spartan_amd.config import FLAGS
    from eigh_ref import EighFakeBackend, eigh_data, same_bits
    backend.set_backend(EighFakeBackend())
    FLAGS.num_workers = W
    runtime.initialize(device='cpu')
    ctx = runtime.get()
    assert ctx.world_size == world and ctx.dist_backend == 'gloo'
    # the gather route: the same bits on both ranks, whatever the layout
    A, _ = eigh_data('gauss', N2, np.float64, 1)
    want = None
    for hint in HINTS2:
      x = expr.from_numpy(A, tile_hint=hint).force()
      if hint != (N2, N2):
        assert {ctx.owner(w) for w in x.tiles.values()} == {0, 1}
      we, ve = expr.eigh(expr.lazify(x))
      wa, va = we.force(), ve.force()
      assert isinstance(wa, distarray.ReplicatedArray) and isinstance(va, distarray.ReplicatedArray)
      w, V = wa.glom(), va.glom()  # this rank's own copy
      _check(A, w, V, 'gloo eigh 2-d %s' % (hint,))
      if want is None:
        want = (w, V)
      assert same_bits(w, want[0]) and same_bits(V, want[1]), hint
    # the slab route and the two cut layouts
    S = _stack(np.float64, 1)
    want = None
    for hint in HINTS3:
      x = expr.from_numpy(S, tile_hint=hint).force()
      if hint != SHAPE3:
        assert {ctx.owner(w) for w in x.tiles.values()} == {0, 1}
      we, ve = expr.eigh(expr.lazify(x))
      va = ve.force()
      assert va.tiles == x.tiles
      w, V = we.glom(), va.glom()
      for b in range(SHAPE3[0]):
        _check(S[b], w[b], V[b], 'gloo eigh 3-d %s matrix %d' % (hint, b))
      if want is None:
        want = (w, V)
      assert same_bits(w, want[0]) and same_bits(V, want[1]), hint
      if hint == SHAPE3:
        continue
      # a NaN in a tile that rank 0 does not own: every rank raises
      e = next(e for e, wk in sorted(x.tiles.items(), key=lambda kv: kv[0].ul) if ctx.owner(wk) == 1)
      bad = S.copy()
      bad[e.ul[0], e.ul[1], e.ul[2]] = np.nan
      bad[e.ul[0], e.ul[2], e.ul[1]] = np.nan
      try:
        expr.eigh(expr.from_numpy(bad, tile_hint=hint))[0].force()
      except np.linalg.LinAlgError as err:
        assert 'Eigenvalues did not converge' in str(err)
      else:
        raise AssertionError('rank %d did not raise for %s' % (rank, hint))
    q.put((rank, 'ok'))
  except Exception:  # pragma: no cover - reported to the parent
    import traceback
    q.put((rank, traceback.format_exc()))
  finally:
    try:
      from spartan_amd import runtime
      runtime.shutdown()
    except Exception:
      pass


@needs_lib
def test_world2_gloo_eigh():
  import multiprocessing as mp
  ctx = mp.get_context('spawn')
  q = ctx.Queue()
  port = _free_port()
  procs = [ctx.Process(target=_gloo_body, args=(r, 2, port, 2, q)) for r in range(2)]
  for p in procs:
    p.start()
  res = {}
  for _ in procs:
    r, msg = q.get(timeout=240)
    res[r] = msg
  for p in procs:
    p.join(timeout=60)
  for r in range(2):
    assert res.get(r) == 'ok', res.get(r)


# ------------------------------------------------------------ ABI, no GPU
@needs_lib
def test_syevj_plan_and_no_launch_cases():
  from spartan_amd import backend
  lib = backend.load_library()
  err = lib.spx_last_error
  for dt, want in ((np.float32, 128), (np.float64, 96)):
    nmax, sweep_max = backend.syevj_plan(dt)
    size = np.dtype(dt).itemsize
    assert (nmax, sweep_max) == (want, 64)
    assert nmax % 32 == 0 and nmax >= backend.geqr_plan(dt, 1)[0]  # ssvd's k x k problem always fits
    # A and V (n columns of n + 1) fit the 160 KiB one workgroup may declare; the next multiple of 32 does not
    assert 2 * nmax * (nmax + 1) * size <= 160 * 1024 < 2 * (nmax + 32) * (nmax + 33) * size
    code = backend.spx_dtype(dt)
    # batch == 0 or n == 0: SPX_OK with no launch, null pointers and all
    for batch, n in ((0, 5), (3, 0), (0, 0)):
      assert lib.spx_syevj(code, 0, batch, n, None, n, n * n, None, n, None, n, n * n, None, None) == 0
  with pytest.raises(TypeError):
    backend.syevj_plan(np.int32)
  assert lib.spx_syevj_plan(1, None, None) == -3 and lib.spx_syevj_plan(99, None, None) == -1
  assert lib.spx_syevj_plan(3, None, None) == 0
  # bad arguments stop at a check (the pointers are host buffers: nothing may launch on them)
  bufs = [(ctypes.c_double * 64)() for _ in range(4)]
  a, w, v, info = (ctypes.cast(b, ctypes.c_void_p) for b in bufs)
  EINVAL, ENOTSUP = -1, -3

  def syevj(dt=4, uplo=0, batch=1, n=4, A=a, lda=4, sa=16, W=w, sw=4, V=v, ldv=4, sv=16, inf=info):
    return lib.spx_syevj(dt, uplo, batch, n, A, lda, sa, W, sw, V, ldv, sv, inf, None)

  assert syevj(dt=99) == EINVAL and b'dtype' in err()
  assert syevj(dt=2) == ENOTSUP and b'float32 / float64' in err()
  assert syevj(uplo=2) == EINVAL and b'uplo' in err()
  assert syevj(batch=-1) == EINVAL and b'negative' in err()
  assert syevj(n=-1) == EINVAL and b'negative' in err()
  assert syevj(dt=3, n=129, lda=129, ldv=129) == ENOTSUP and b'limit 128' in err()
  assert syevj(dt=4, n=97, lda=97, ldv=97) == ENOTSUP and b'limit 96' in err()
  for name in ('A', 'W', 'V', 'inf'):
    assert syevj(**{name: None}) == EINVAL and b'null' in err()
  assert syevj(lda=3) == EINVAL and b'leading dimension' in err()
  assert syevj(ldv=3) == EINVAL and b'leading dimension' in err()
  assert syevj(batch=2, sw=3) == EINVAL and b'overlap' in err()
  assert syevj(batch=2, sv=15) == EINVAL and b'overlap' in err()
  assert syevj(batch=2, sa=-1) == EINVAL and b'stride_a' in err()


# ---------------------------------------------------------------- the model
def test_round_robin_meets_every_pair_once():
  from eigh_ref import round_robin
  for n in list(range(2, 10)) + [17]:
    m = n + (n & 1)
    rounds = round_robin(m)
    assert len(rounds) == m - 1
    seen = []
    for pairs in rounds:
      assert len(pairs) == m // 2
      assert sorted(i for pq in pairs for i in pq) == list(range(m))  # disjoint, and everyone plays
      seen.extend(pairs)
    assert sorted(seen) == [(p, q) for p in range(m) for q in range(p + 1, m)]  # every pair exactly once


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_model_converges_inside_the_envelope(dtype):
  """The model half of the yardstick: it converges within sweep_max, its
  orthogonality stays inside the unconditional envelope, its exact cases are
  exact, and it stays within FACTOR of itself across two seeds."""
  from eigh_ref import FACTOR, KINDS, SWEEP_MAX, eigh_data, envelope, jacobi_model, model_run, yardstick
  for n in (1, 2, 3, 4, 5, 17, 33, 64):
    worst = [[0.0] * 3, [0.0] * 3]
    for seed in (0, 1):
      for kind in KINDS:
        (res, orth, ev), sweeps = model_run(kind, n, dtype, seed)
        assert 0 <= sweeps <= SWEEP_MAX
        if sweeps == 0:
          assert orth == 0
        else:
          assert orth <= envelope(n, sweeps), (kind, n, seed, orth, sweeps)
        if kind == 'zero' or n == 1:
          assert sweeps == 0 and res == 0
        if kind == 'diag' and n > 1:
          assert sweeps == 1 and res == 0 and orth == 0 and ev == 0
        if kind == 'exchange' and n > 1:
          assert ev == 0 and res == 0  # eigenvalues exactly +-1
        for i, x in enumerate((res, orth, ev)):
          if x is not None:
            worst[seed][i] = max(worst[seed][i], x)
    print('model %s n=%d: seed 0 %s, seed 1 %s, yardstick %s' % (np.dtype(dtype), n, worst[0], worst[1],
                                                               yardstick(dtype, n)))
    # (rounding the prescribed matrix to the dtype alone moves a ratio by up to 1 u: below that a ratio says
    # nothing about the method, so the comparison starts there)
    for a, b in zip(*worst):
      assert a <= FACTOR * max(b, 1.0) and b <= FACTOR * max(a, 1.0), (n, worst)
  A, _ = eigh_data('gauss', 5, dtype)
  A[3, 1] = A[1, 3] = np.nan
  w, V, sweeps = jacobi_model(A)
  assert sweeps == -1 and np.all(np.isnan(w)) and np.all(np.isnan(V))


# --------------------------------------------------------------- the drivers
@needs_lib
@pytest.mark.parametrize('W', [1, 3])
def test_reference_svds_and_lanczos(eigh_ctx, W):
  eigh_ctx(W)
  from eigh_ref import check_drivers
  check_drivers(W)
