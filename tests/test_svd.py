"""``spartan_amd.svd`` / ``svdvals`` / ``pinv`` host logic (no GPU): every route
of the expression layer over tile layouts and worker counts, laziness,
validation, LinAlgError, two gloo ranks, the plan / no-launch answers of
spx_gesvj, and the NumPy model that is half of the yardstick.

The expression layer runs here over the CPU test double with a scipy ``gesvj``
(svd_ref.SvdFakeBackend); the kernel itself is tested on the GPU in
tests/test_svd_gpu.py.
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

M2, N2 = 13, 10
HINTS2 = [(13, 10), (4, 10), (13, 3), (4, 3)]  # one tile; row slabs; column cuts; 2-d cuts
SHAPE3 = (7, 8, 6)
HINTS3 = [(7, 8, 6), (2, 8, 6), (3, 5, 6), (2, 8, 2)]  # one tile; batch slabs; two layouts cut inside the matrices
SLAB_HINTS = [(7, 8, 6), (2, 8, 6)]
LDS = 160 * 1024


@pytest.fixture
def svd_ctx(host_ctx):
  """host_ctx with the svd-capable test double installed."""
  from spartan_amd import backend
  from svd_ref import SvdFakeBackend

  def make(num_workers=1):
    host_ctx(num_workers)
    be = SvdFakeBackend()
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


def _stack(dtype, shape=SHAPE3, seed=0):
  """One matrix of seven different kinds."""
  from svd_ref import svd_data
  kinds = ('gauss', 'illcond', 'rankdef', 'diag', 'zero', 'cluster', 'dup')
  return np.stack([svd_data(k, shape[1], shape[2], dtype, seed)[0] for k in kinds[:shape[0]]])


def _check(A, U, s, Vt, what, yard=None):
  """The reduced triple of ``A`` (either orientation) in the contract's form.
  The test double is LAPACK: its ratios stay within the margin of the
  yardstick (``yard``; default: the direct route's)."""
  from svd_ref import FACTOR, check_form, svd_ratios, yardstick
  m, n = A.shape
  k = min(m, n)
  assert U.shape == (m, k) and s.shape == (k,) and Vt.shape == (k, n), what
  assert U.dtype == A.dtype and s.dtype == A.dtype and Vt.dtype == A.dtype, what
  if m < n:  # the transposed problem: the square factor is U
    A, U, Vt = A.T, Vt.T, U.T
  check_form(s, Vt)
  yard = yard or yardstick(A.dtype, *A.shape)
  res, orthV, orthU, _ = svd_ratios(np.ascontiguousarray(A), np.ascontiguousarray(U), s, np.ascontiguousarray(Vt))
  print('%s: res %.3g u (yardstick %.3g), orthV %.3g u (%.3g), orthU %.3g u (%.3g)'
        % (what, res, yard[0], orthV, yard[1], orthU, yard[2]))
  assert res <= FACTOR * yard[0] and orthV <= FACTOR * yard[1] and orthU <= FACTOR * yard[2], what


def _force3(triple):
  return tuple(e.force() for e in triple)


# ------------------------------------------------------------- expr layer
@needs_lib
@pytest.mark.parametrize('W', [1, 3])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_svd_2d_direct_every_layout(svd_ctx, gathers, W, dtype):
  be = svd_ctx(W)
  from spartan_amd import expr
  from spartan_amd.array import distarray
  from svd_ref import same_bits, svd_data
  A, _ = svd_data('gauss', M2, N2, dtype)
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
    arrs = _force3(expr.svd(x))
    assert all(isinstance(a, distarray.ReplicatedArray) for a in arrs), hint
    assert be.calls.count('gesvj') == 1 and 'geqr' not in be.calls, hint  # one backend call per forced triple
    assert len(gathers) == (0 if hint == 'replicated' else 1), hint  # ONE exchange of the whole matrix
    U, s, Vt = (a.glom() for a in arrs)
    _check(A, U, s, Vt, 'svd 2-d %s W=%d %s' % (hint, W, np.dtype(dtype)))
    if first is None:
      first = (U, s, Vt)
    assert all(same_bits(a, b) for a, b in zip((U, s, Vt), first)), hint  # the same bits for every layout
  # wide, both ways: the expression's transpose and a wide array of its own
  At = np.ascontiguousarray(A.T)
  for x in (expr.transpose(expr.from_numpy(A, tile_hint=(4, 3))), expr.from_numpy(At, tile_hint=(3, 4)), At,
            _replicated(At)):
    del be.calls[:]
    Ue, se, Vte = expr.svd(x)
    assert Ue.shape == (N2, N2) and se.shape == (N2,) and Vte.shape == (N2, M2)
    U, s, Vt = Ue.glom(), se.glom(), Vte.glom()
    assert be.calls.count('gesvj') == 1
    _check(At, U, s, Vt, 'svd wide W=%d' % W)
    # svd(transpose(A)) is (Vt^T, s, U^T) of svd(A), bit for bit
    assert same_bits(U, np.ascontiguousarray(first[2].T)) and same_bits(s, first[1])
    assert same_bits(Vt, np.ascontiguousarray(first[0].T))
  # svdvals: the same bits, U and Vt never formed
  del be.calls[:]
  assert same_bits(expr.svdvals(expr.from_numpy(A, tile_hint=(4, 3))).glom(), first[1])
  assert same_bits(expr.svd(At, compute_uv=False).glom(), first[1])
  assert be.calls.count('gesvj') == 2


def _tall_limit(monkeypatch, mmax):
  """Makes the direct route end at ``mmax`` rows, so that small matrices take
  the tall route (the plan's nmax and sweep_max stay the library's)."""
  from spartan_amd import backend
  real = backend.gesvj_plan

  def plan(dtype, n):
    nmax, m, sweeps = real(dtype, n)
    return nmax, min(m, mmax), sweeps
  monkeypatch.setattr(backend, 'gesvj_plan', plan)


@needs_lib
@pytest.mark.parametrize('W', [1, 3])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_svd_2d_tall_and_wide_routes(svd_ctx, gathers, monkeypatch, W, dtype):
  be = svd_ctx(W)
  _tall_limit(monkeypatch, 12)
  from spartan_amd import expr
  from spartan_amd.array import distarray
  from svd_ref import same_bits, svd_data, tall_yardstick
  m, n = 40, 6
  for kind in ('gauss', 'rankdef'):
    A, _ = svd_data(kind, m, n, dtype)
    want = np.linalg.svd(A.astype(np.float64), compute_uv=False)
    # row slabs; a last slab of fewer than n rows (40 = 3 * 12 + 4); column cuts; 2-d cuts; replicated
    for hint in [(m, n), (14, n), (12, n), (m, 4), (14, 4), 'replicated']:
      x = _replicated(A) if hint == 'replicated' else expr.lazify(expr.from_numpy(A, tile_hint=hint).force())
      del be.calls[:]
      Ua, sa, Vta = _force3(expr.svd(x))
      assert be.calls.count('gesvj') == 1 and be.calls.count('geqr') >= 1, hint
      assert isinstance(sa, distarray.ReplicatedArray) and isinstance(Vta, distarray.ReplicatedArray), hint
      if hint == 'replicated':
        assert isinstance(Ua, distarray.ReplicatedArray)
      elif hint in [(14, n), (12, n)]:
        assert Ua.tiles == x.force().tiles, hint  # U is tiled like A: no row left its owner
      U, s, Vt = Ua.glom(), sa.glom(), Vta.glom()
      # (QR first, then the SVD of R: held to the sum of the two yardsticks, svd_ref.tall_yardstick)
      _check(A, U, s, Vt, 'svd tall %s %s W=%d %s' % (kind, hint, W, np.dtype(dtype)), tall_yardstick(dtype, m, n))
      np.testing.assert_allclose(s, want, rtol=0, atol=want[0] * 64 * np.finfo(dtype).eps)
      # the wide mirror: the same layout transposed
      del be.calls[:]
      xt = _replicated(np.ascontiguousarray(A.T)) if hint == 'replicated' else expr.transpose(x)
      Ue, se, Vte = expr.svd(xt)
      assert Ue.shape == (n, n) and se.shape == (n,) and Vte.shape == (n, m)
      U2, s2, Vt2 = Ue.glom(), se.glom(), Vte.glom()
      assert be.calls.count('gesvj') == 1
      assert same_bits(U2, np.ascontiguousarray(Vt.T)) and same_bits(s2, s), hint
      assert same_bits(Vt2, np.ascontiguousarray(U.T)), hint
    del be.calls[:]
    s = expr.svdvals(expr.from_numpy(A, tile_hint=(14, n))).glom()
    np.testing.assert_allclose(s, want, rtol=0, atol=want[0] * 64 * np.finfo(dtype).eps)
    assert 'orgqr' not in be.calls or be.calls.count('gesvj') == 1


@needs_lib
@pytest.mark.parametrize('W', [1, 3])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_svd_3d_every_route(svd_ctx, gathers, W, dtype):
  be = svd_ctx(W)
  import torch
  from spartan_amd import expr
  from spartan_amd.array import distarray
  from svd_ref import same_bits
  nb, m, n = SHAPE3
  for shape, hints in ((SHAPE3, HINTS3), ((nb, n, m), [tuple(h[i] for i in (0, 2, 1)) for h in HINTS3])):
    A = _stack(dtype)
    if shape != SHAPE3:
      A = np.ascontiguousarray(A.transpose(0, 2, 1))  # a stack of wide matrices
    k = min(shape[1:])
    first = None
    for hint in hints + ['replicated']:
      x = distarray.ReplicatedArray(torch.as_tensor(A.copy())) if hint == 'replicated' \
          else expr.from_numpy(A, tile_hint=hint).force()
      del be.calls[:]
      del gathers[:]
      Ue, se, Vte = expr.svd(expr.lazify(x))
      assert Ue.shape == (nb, shape[1], k) and se.shape == (nb, k) and Vte.shape == (nb, k, shape[2])
      arrs = _force3((Ue, se, Vte))
      if hint == 'replicated':
        assert all(isinstance(a, distarray.ReplicatedArray) for a in arrs)
        assert be.calls.count('gesvj') == 1 and not gathers
      else:
        cuts = sorted({(e.ul[0], e.lr[0]) for e in x.tiles})
        for a in arrs:  # U, s and Vt are cut along axis 0 at the slab cuts, whole otherwise
          assert sorted((e.ul[0], e.lr[0]) for e in a.tiles) == cuts, hint
          assert all(e.ul[1:] == (0,) * (a.ndim - 1) and tuple(e.lr[1:]) == tuple(a.shape[1:]) for e in a.tiles)
        slab = tuple(hint[i] for i in ((0, 2, 1) if shape != SHAPE3 else (0, 1, 2))) in SLAB_HINTS
        if slab:
          assert be.calls.count('gesvj') == len(x.tiles) and not gathers, hint  # one call per tile, no exchange
          for e, wk in x.tiles.items():  # on the same workers
            for a in arrs:
              assert [w for t, w in a.tiles.items() if t.ul[0] == e.ul[0]] == [wk]
        else:
          assert be.calls.count('gesvj') == len(cuts) and len(gathers) == 1, hint  # one call per slab, one exchange
      U, s, Vt = (a.glom() for a in arrs)
      for b in range(nb):
        _check(A[b], U[b], s[b], Vt[b], 'svd 3-d %s W=%d matrix %d' % (hint, W, b))
      if first is None:
        first = (U, s, Vt)
      assert all(same_bits(a, b) for a, b in zip((U, s, Vt), first)), hint
    sv = expr.svdvals(expr.from_numpy(A, tile_hint=hints[1]))
    assert sv.shape == (nb, k) and same_bits(sv.glom(), first[1])


@needs_lib
def test_lazy_shape_dtype_and_one_call(svd_ctx):
  be = svd_ctx(3)
  from spartan_amd import expr
  from svd_ref import svd_data
  A, _ = svd_data('gauss', M2, N2, np.float64, 3)
  Ue, se, Vte = expr.svd(expr.from_numpy(A, tile_hint=(4, 3)))
  assert all(isinstance(e, expr.Expr) for e in (Ue, se, Vte))
  assert Ue.shape == (M2, N2) and se.shape == (N2,) and Vte.shape == (N2, N2)
  assert Ue.dtype == np.float64 and se.dtype == np.float64 and Vte.dtype == np.float64
  prod = expr.dot(Ue * se, Vte)  # U diag(s) Vt, still lazy
  assert 'gesvj' not in be.calls
  s = se.glom()
  assert be.calls.count('gesvj') == 1
  U, Vt = Ue.glom(), Vte.glom()
  assert be.calls.count('gesvj') == 1  # the triple shares one evaluation
  np.testing.assert_allclose(prod.glom(), A, atol=1e-12)
  assert be.calls.count('gesvj') == 1
  U2, s2, Vt2 = np.linalg.svd(A, full_matrices=False)
  np.testing.assert_allclose(s, s2, atol=1e-12)
  np.testing.assert_allclose(np.abs(U), np.abs(U2), atol=1e-10)
  np.testing.assert_allclose(np.abs(Vt), np.abs(Vt2), atol=1e-10)
  sv = expr.svdvals(np.ones((3, 5), np.float32))
  assert isinstance(sv, expr.Expr) and sv.shape == (3,) and sv.dtype == np.float32


@needs_lib
@pytest.mark.parametrize('W', [1, 3])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_pinv(svd_ctx, W, dtype):
  svd_ctx(W)
  from spartan_amd import expr
  from svd_ref import svd_data
  eps = np.finfo(dtype).eps
  for (m, n), kind in (((13, 10), 'gauss'), ((13, 10), 'rankdef'), ((6, 6), 'illcond'), ((9, 4), 'zero')):
    A, _ = svd_data(kind, m, n, dtype)
    for M, hint in ((A, (4, n)), (np.ascontiguousarray(A.T), (n, 4))):  # tall and wide
      P = expr.pinv(expr.from_numpy(M, tile_hint=hint))
      assert isinstance(P, expr.Expr) and P.shape == M.shape[::-1] and P.dtype == np.dtype(dtype)
      got = P.glom()
      want = np.linalg.pinv(M.astype(np.float64), rcond=max(m, n) * eps)
      if kind == 'zero':
        assert not np.any(got)
        continue
      s = np.linalg.svd(M.astype(np.float64), compute_uv=False)
      live = s[s > max(m, n) * eps * s[0]]
      # |pinv(A + E) - pinv(A)| <= about 3 |pinv|^2 |E| for perturbations that keep the rank (Wedin)
      bound = 3 * 16 * max(m, n) * eps * s[0] / live[-1] ** 2
      assert np.abs(got - want).max() <= bound, (kind, m, n, np.abs(got - want).max(), bound)
  A, _ = svd_data('gauss', 8, 5, dtype)
  got = expr.pinv(A, rcond=0.5).glom()  # an explicit cut: the small singular values are dropped
  np.testing.assert_allclose(got, np.linalg.pinv(A.astype(np.float64), rcond=0.5), atol=64 * eps)


@needs_lib
def test_validation_errors(svd_ctx):
  svd_ctx(1)
  from spartan_amd import backend, expr
  for bad in (np.ones(4), np.ones((2, 2, 3, 3))):
    with pytest.raises(ValueError, match='matrix'):
      expr.svd(bad)
  with pytest.raises(ValueError, match='2-d'):
    expr.pinv(np.ones((2, 3, 3)))
  with pytest.raises(TypeError, match='float32 / float64'):
    expr.svd(np.ones((4, 4), np.int64))
  with pytest.raises(TypeError, match='float32 / float64'):
    expr.svdvals(np.ones((4, 4), np.float16))
  with pytest.raises(NotImplementedError, match='full_matrices'):
    expr.svd(np.ones((4, 3)), full_matrices=True)
  sp = expr.sparse_diagonal((6, 6), dtype=np.float64)
  for f in (expr.svd, expr.svdvals, expr.pinv):
    with pytest.raises(TypeError, match='todense'):
      f(sp)
  for dt in (np.float32, np.float64):
    nmax, mmax, _ = backend.gesvj_plan(dt, 6)
    qmax = backend.geqr_plan(dt, 1)[0]
    lim = min(nmax, qmax)  # the tall route ends at the smaller column limit
    # a stack beyond one workgroup; a tall matrix of more columns than qr takes, both ways
    with pytest.raises(NotImplementedError, match='stack'):
      expr.svd(np.ones((2, mmax + 1, 6), dt))
    with pytest.raises(NotImplementedError, match='stack'):
      expr.svdvals(np.ones((2, 6, mmax + 1), dt))
    with pytest.raises(NotImplementedError, match='limits of %d .svd. and %d .qr.' % (nmax, qmax)):
      expr.svd(np.ones((4 * nmax, lim + 1), dt))
    with pytest.raises(NotImplementedError, match='limits of %d .svd. and %d .qr.' % (nmax, qmax)):
      expr.svd(np.ones((lim + 1, 4 * nmax), dt))
    expr.svd(np.ones((nmax, nmax), dt))  # the limits themselves are accepted
    expr.svd(np.ones((2, mmax, 6), dt))
    expr.svd(np.ones((mmax + 1, 6), dt))  # the tall route


@needs_lib
@pytest.mark.parametrize('W', [1, 3])
def test_linalg_error(svd_ctx, monkeypatch, W):
  svd_ctx(W)
  from spartan_amd import expr
  from svd_ref import svd_data
  A, _ = svd_data('gauss', M2, N2, np.float64)
  A[7, 2] = np.nan
  for hint in HINTS2:
    with pytest.raises(np.linalg.LinAlgError, match='SVD did not converge'):
      expr.svd(expr.from_numpy(A, tile_hint=hint))[0].force()
  with pytest.raises(np.linalg.LinAlgError, match='SVD did not converge'):
    expr.svdvals(_replicated(A)).force()
  with pytest.raises(np.linalg.LinAlgError, match='SVD did not converge'):
    expr.pinv(A.T).force()
  S = _stack(np.float64)
  S[5, 3, 1] = np.inf
  for hint in HINTS3:
    with pytest.raises(np.linalg.LinAlgError, match='SVD did not converge'):
      expr.svd(expr.from_numpy(S, tile_hint=hint))[1].force()
  _tall_limit(monkeypatch, 12)  # the tall route: the NaN reaches R
  B, _ = svd_data('gauss', 40, 6, np.float64)
  B[17, 3] = np.nan
  with pytest.raises(np.linalg.LinAlgError, match='SVD did not converge'):
    expr.svd(expr.from_numpy(B, tile_hint=(14, 6)))[2].force()


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
    from svd_ref import SvdFakeBackend, same_bits, svd_data, tall_yardstick
    backend.set_backend(SvdFakeBackend())
    FLAGS.num_workers = W
    runtime.initialize(device='cpu')
    ctx = runtime.get()
    assert ctx.world_size == world and ctx.dist_backend == 'gloo'
    # the direct route: the same bits on both ranks, whatever the layout, tall and wide
    A, _ = svd_data('gauss', M2, N2, np.float64, 1)
    want = None
    for hint in HINTS2:
      x = expr.from_numpy(A, tile_hint=hint).force()
      if hint != (M2, N2):
        assert {ctx.owner(w) for w in x.tiles.values()} == {0, 1}
      arrs = tuple(e.force() for e in expr.svd(expr.lazify(x)))
      assert all(isinstance(a, distarray.ReplicatedArray) for a in arrs)
      got = tuple(a.glom() for a in arrs)  # this rank's own copy
      _check(A, *got, what='gloo svd 2-d %s' % (hint,))
      if want is None:
        want = got
      assert all(same_bits(a, b) for a, b in zip(got, want)), hint
      Ut, st, Vtt = (e.glom() for e in expr.svd(expr.transpose(expr.lazify(x))))
      assert same_bits(Ut, np.ascontiguousarray(want[2].T)) and same_bits(st, want[1])
      assert same_bits(Vtt, np.ascontiguousarray(want[0].T))
    # the tall route (the direct limit lowered), over row slabs and a column-cut layout
    real = backend.gesvj_plan
    backend.gesvj_plan = lambda dt, n: (real(dt, n)[0], min(real(dt, n)[1], 12), real(dt, n)[2])
    try:
      B, _ = svd_data('illcond', 40, 6, np.float64, 1)
      for hint in [(14, 6), (12, 6), (14, 4)]:
        x = expr.from_numpy(B, tile_hint=hint).force()
        assert {ctx.owner(w) for w in x.tiles.values()} == {0, 1}
        U, s, Vt = (e.glom() for e in expr.svd(expr.lazify(x)))
        _check(B, U, s, Vt, 'gloo svd tall %s' % (hint,), tall_yardstick(np.float64, 40, 6, 1))
        P = expr.pinv(expr.lazify(x)).glom()
        np.testing.assert_allclose(P.dot(B), np.eye(6), atol=1e-3)  # cond 1e13: P B = I to cond u
      bad = B.copy()
      bad[39, 5] = np.nan  # in the last slab, which rank 0 does not own
      try:
        expr.svdvals(expr.from_numpy(bad, tile_hint=(14, 6))).force()
      except np.linalg.LinAlgError as err:
        assert 'SVD did not converge' in str(err)
      else:
        raise AssertionError('rank %d did not raise on the tall route' % rank)
    finally:
      backend.gesvj_plan = real
    # the stack: slabs and a cut layout; a NaN in a tile that rank 0 does not own raises everywhere
    S = _stack(np.float64, seed=1)
    want = None
    for hint in HINTS3:
      x = expr.from_numpy(S, tile_hint=hint).force()
      if hint != SHAPE3:
        assert {ctx.owner(w) for w in x.tiles.values()} == {0, 1}
      got = tuple(e.glom() for e in expr.svd(expr.lazify(x)))
      for b in range(SHAPE3[0]):
        _check(S[b], got[0][b], got[1][b], got[2][b], 'gloo svd 3-d %s matrix %d' % (hint, b))
      if want is None:
        want = got
      assert all(same_bits(a, b) for a, b in zip(got, want)), hint
      if hint == SHAPE3:
        continue
      e = next(e for e, wk in sorted(x.tiles.items(), key=lambda kv: kv[0].ul) if ctx.owner(wk) == 1)
      bad = S.copy()
      bad[e.ul[0], e.ul[1], e.ul[2]] = np.nan
      try:
        expr.svd(expr.from_numpy(bad, tile_hint=hint))[1].force()
      except np.linalg.LinAlgError as err:
        assert 'SVD did not converge' in str(err)
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
def test_world2_gloo_svd():
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
def _lds_bytes(size, m, n, jobu=1):
  """The documented layout: 16 doubles of reduction scratch, G
  in n columns of m | 1, V in n columns of n | 1 (jobu only), the singular
  values and signs (2 n), the permutation (n ints) and the 16-byte flag."""
  return 16 * 8 + (n * (m | 1) + (n * (n | 1) if jobu else 0) + 2 * n) * size + 4 * n + 16


@needs_lib
def test_gesvj_plan_and_no_launch_cases():
  from spartan_amd import backend
  lib = backend.load_library()
  err = lib.spx_last_error
  for dt, want in ((np.float32, 128), (np.float64, 96)):
    size = np.dtype(dt).itemsize
    nmax = max(n for n in range(32, 513, 32) if _lds_bytes(size, n, n) <= LDS)
    assert nmax == want
    for n in (1, 2, 5, 17, 64, nmax - 1, nmax, nmax + 1, 4 * nmax):
      got = backend.gesvj_plan(dt, n)
      mmax = 0 if n > nmax else max(m for m in range(n, LDS) if _lds_bytes(size, m, n) <= LDS)
      assert got == (nmax, mmax, 64), (dt, n, got, mmax)
      if mmax:
        assert mmax >= n and _lds_bytes(size, mmax + 1, n) > LDS
    assert backend.gesvj_plan(dt, 0)[0] == nmax
    assert nmax >= backend.geqr_plan(dt, 1)[0]  # the R of every qr fits
    code = backend.spx_dtype(dt)
    # batch == 0 or n == 0: SPX_OK with no launch, null pointers and all
    for batch, m, n in ((0, 7, 5), (3, 4, 0), (3, 0, 0), (0, 0, 0)):
      assert lib.spx_gesvj(code, 1, batch, m, n, None, n, m * n, None, n, m * n, None, n, None, n, n * n, None,
                           None) == 0
  with pytest.raises(TypeError):
    backend.gesvj_plan(np.int32, 4)
  with pytest.raises(ValueError, match='negative'):
    backend.gesvj_plan(np.float32, -1)
  assert lib.spx_gesvj_plan(1, 4, None, None, None) == -3 and lib.spx_gesvj_plan(99, 4, None, None, None) == -1
  assert lib.spx_gesvj_plan(3, 4, None, None, None) == 0 and lib.spx_gesvj_plan(3, -1, None, None, None) == -1
  # bad arguments stop at a check (the pointers are host buffers: nothing may launch on them)
  bufs = [(ctypes.c_double * 64)() for _ in range(5)]
  a, u, s, vt, info = (ctypes.cast(b, ctypes.c_void_p) for b in bufs)
  EINVAL, ENOTSUP = -1, -3

  def gesvj(dt=4, jobu=1, batch=1, m=5, n=4, A=a, lda=4, sa=20, U=u, ldu=4, su=20, S=s, ss=4, Vt=vt, ldvt=4, svt=16,
            inf=info):
    return lib.spx_gesvj(dt, jobu, batch, m, n, A, lda, sa, U, ldu, su, S, ss, Vt, ldvt, svt, inf, None)

  assert gesvj(dt=99) == EINVAL and b'dtype' in err()
  assert gesvj(dt=2) == ENOTSUP and b'float32 / float64' in err()
  assert gesvj(jobu=2) == EINVAL and b'jobu' in err()
  assert gesvj(batch=-1) == EINVAL and b'negative' in err()
  assert gesvj(m=-1) == EINVAL and b'negative' in err()
  assert gesvj(n=-1) == EINVAL and b'negative' in err()
  assert gesvj(m=3) == EINVAL and b'below n' in err()
  assert gesvj(dt=3, m=129, n=129, lda=129, ldu=129, ldvt=129) == ENOTSUP and b'limit 128' in err()
  assert gesvj(dt=4, m=97, n=97, lda=97, ldu=97, ldvt=97) == ENOTSUP and b'limit 96' in err()
  for dt, code in ((np.float32, 3), (np.float64, 4)):
    mmax = backend.gesvj_plan(dt, 4)[1]
    assert gesvj(dt=code, m=mmax + 1) == ENOTSUP and b'limit %d for n = 4' % mmax in err()
    mmax0 = max(m for m in range(4, LDS) if _lds_bytes(np.dtype(dt).itemsize, m, 4, 0) <= LDS)
    assert mmax0 > mmax  # jobu == 0 holds no V: more rows fit
    assert gesvj(dt=code, jobu=0, m=mmax0 + 1, U=None, Vt=None) == ENOTSUP and b'limit %d for n = 4' % mmax0 in err()
  assert gesvj(batch=1 << 31) == ENOTSUP and b'2^31' in err()
  for name in ('A', 'U', 'S', 'Vt', 'inf'):
    assert gesvj(**{name: None}) == EINVAL and b'null' in err()
  assert gesvj(jobu=0, Vt=None) == EINVAL and b'null' in err()  # U and Vt are NULL iff jobu == 0
  assert gesvj(jobu=0, U=None) == EINVAL and b'null' in err()
  for name in ('lda', 'ldu', 'ldvt'):
    assert gesvj(**{name: 3}) == EINVAL and b'leading dimension' in err()
  assert gesvj(batch=2, ss=3) == EINVAL and b'overlap' in err()
  assert gesvj(batch=2, su=19) == EINVAL and b'overlap' in err()
  assert gesvj(batch=2, svt=15) == EINVAL and b'overlap' in err()
  assert gesvj(batch=2, sa=-1) == EINVAL and b'stride_a' in err()


# ---------------------------------------------------------------- the model
def gpu_sizes(dtype):
  """The (m, n) of tests/test_svd_gpu.py::test_gesvj."""
  from spartan_amd import backend
  nmax = backend.gesvj_plan(dtype, 1)[0]
  sq = [1, 2, 3, 4, 5, 17, 63, 64, 65, nmax - 1, nmax]
  return [(n, n) for n in sq] + [(2, 1), (65, 17), (backend.gesvj_plan(dtype, 17)[1], 17),
                                 (backend.gesvj_plan(dtype, 64)[1], 64)]


@needs_lib
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_model_converges_inside_the_envelope(dtype):
  """The model half of the yardstick, at every size the GPU test uses: it
  converges within sweep_max on every kind, its orthV stays inside the
  unconditional envelope, and its exact cases are exact."""
  from svd_ref import KINDS, SWEEP_MAX, dup_columns, envelope, jacobi_svd_model, model_run, svd_data, yardstick
  most = (-1, ())
  for m, n in gpu_sizes(dtype):
    for kind in KINDS:
      (res, orthV, orthU, sv), sweeps, s = model_run(kind, m, n, dtype)
      assert 0 <= sweeps <= SWEEP_MAX, (kind, m, n, sweeps)
      most = max(most, (sweeps, (kind, m, n)))
      if sweeps == 0:
        assert orthV == 0
      else:
        assert orthV <= envelope(n, sweeps), (kind, m, n, orthV, sweeps)
      if kind == 'zero' or n == 1:
        assert sweeps == 0
      if kind == 'zero':
        assert res == 0 and not np.any(s)
      if kind == 'diag' and n > 1:
        assert sweeps == 1 and res == 0 and orthV == 0 and orthU == 0 and sv == 0  # s = sorted |d| exactly
      if kind == 'dup' and n > 1:
        assert np.count_nonzero(s == 0) == (1 if dup_columns(n)[2] is None else 2), (m, n, s)
      if kind == 'ones' and n > 1:
        assert np.count_nonzero(s == 0) == n - 1, (m, n, s)
    print('model %s (%d, %d): yardstick %s, sweeps %s' % (np.dtype(dtype), m, n, ['%.3g' % y for y in yardstick(dtype, m, n)],
                                                         [model_run(k, m, n, dtype)[1] for k in KINDS]))
  print('model %s: at most %d sweeps, on %s' % (np.dtype(dtype), most[0], most[1]))
  A, _ = svd_data('gauss', 7, 5, dtype)
  A[3, 1] = np.nan
  U, s, Vt, sweeps = jacobi_svd_model(A)
  assert sweeps == -1 and np.all(np.isnan(U)) and np.all(np.isnan(s)) and np.all(np.isnan(Vt))


@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_model_relative_accuracy_on_graded_columns(dtype):
  """The reason for a one-sided method: on column-graded data the model keeps
  every singular value to a modest multiple of u RELATIVE to itself, over a
  grading of 1e6 (float32) / 1e15 (float64).  (LAPACK's gesvd is printed
  beside it, not asserted: it promises the norm-wise bound only.)"""
  from svd_ref import lapack_svd, rel_ratio, rel_reference, svd_data
  for m, n in ((17, 17), (65, 17), (64, 64)):
    ref = rel_reference(m, n, dtype)
    if ref is None:
      pytest.skip('np.longdouble is not wider than float64 here: nothing to compare float64 against')
    sigma, model = ref
    A, _ = svd_data('graded', m, n, dtype)
    lapack = rel_ratio(lapack_svd(A)[1], sigma, dtype)
    print('graded %s (%d, %d): rel %.3g u (model), %.3g u (gesvd)' % (np.dtype(dtype), m, n, model, lapack))
    # a random walk over about sweeps * n rotations of relative error u each stays below n * sqrt(n) u
    assert model <= n * np.sqrt(n), (m, n, model)
