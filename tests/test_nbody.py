"""``spartan_amd.nbody_accel`` and ``examples.nbody`` host logic (no GPU): the
yardstick's own identities, the pinned divergence from the reference's
``set_diagonal``, every layout of the expression layer over worker counts,
laziness and sharing, the refusals, the driver against a NumPy loop, and the
plan answers and argument checks of spx_nbody_plan / spx_nbody_accel.

The expression layer runs here over the CPU test double whose ``nbody_accel``
is the yardstick (nbody_ref.NbodyFakeBackend); the kernel itself is tested on
the GPU in tests/test_nbody_gpu.py.
"""
import ctypes
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB = os.path.join(ROOT, 'spartan_amd', 'libspx.so')

needs_lib = pytest.mark.skipif(not os.path.exists(LIB), reason='libspx.so not built')

N = 10


@pytest.fixture
def nbody_ctx(host_ctx):
  """host_ctx with the n-body-capable test double installed."""
  from spartan_amd import backend
  from nbody_ref import NbodyFakeBackend

  def make(num_workers=1):
    host_ctx(num_workers)
    be = NbodyFakeBackend()
    backend.set_backend(be)
    return be
  return make


# --------------------------------------------------------------- yardstick
def test_yardstick_identities():
  from nbody_ref import nbody_ref, unit_galaxy
  # one body: exact zeros
  a, S = nbody_ref([3.0], [4.0], [5.0], [2.0], 1.5, 1.0)
  assert np.array_equal(a, np.zeros((3, 1))) and np.array_equal(S, np.zeros((3, 1)))
  # two bodies: G m / r^2 along the separation, towards each other
  G, m = 2.0, np.array([3.0, 5.0])
  p = np.array([[0.0, 0.0, 0.0], [3.0, 4.0, 12.0]])  # r = 13
  a, _S = nbody_ref(p[:, 0], p[:, 1], p[:, 2], m, G, 1.0)
  u = (p[1] - p[0]) / 13.0
  np.testing.assert_allclose(a[:, 0], G * m[1] / 169.0 * u, rtol=1e-14)
  np.testing.assert_allclose(a[:, 1], -G * m[0] / 169.0 * u, rtol=1e-14)
  assert np.all(np.sign(a[:, 0]) == -np.sign(a[:, 1]))
  # momentum: sum_j m_j a_j = 0 within the rounding of the terms
  x, y, z, m = unit_galaxy(300, np.float64)
  a, S = nbody_ref(x, y, z, m, 1.0, 1.0)
  assert np.all(np.abs((m * a).sum(axis=1)) <= 1e-12 * (m * S).sum(axis=1))
  # two bodies at one position exert exactly nothing on each other; a third still pulls both
  a, _S = nbody_ref([1.0, 1.0, 9.0], [2.0, 2.0, 2.0], [3.0, 3.0, 3.0], [5.0, 7.0, 0.0], 1.0, 1.0)
  assert np.array_equal(a[:, :2], np.zeros((3, 2)))
  a, _S = nbody_ref([1.0, 1.0, 9.0], [2.0, 2.0, 2.0], [3.0, 3.0, 3.0], [5.0, 7.0, 11.0], 1.0, 1.0)
  assert a[0, 0] == a[0, 1] == 11.0 * 8.0 / 512.0 and np.array_equal(a[1:], np.zeros((2, 3)))
  # a separation below rmin: G m d / rmin^3
  a, _S = nbody_ref([0.0, 0.25], [0.0, 0.0], [0.0, 0.0], [3.0, 5.0], 2.0, 2.0)
  assert a[0, 0] == 2.0 * 5.0 * 0.25 / 8.0 and a[0, 1] == -2.0 * 3.0 * 0.25 / 8.0


def test_reference_set_diagonal_replaces_the_whole_first_strip():
  """The divergence pin.  The reference's ``_set_diagonal_mapper`` returns the
  scalar in place of the tile whenever the tile's upper-left corner is on the
  diagonal.  With two row strips of an (8, 8) array that replaces ALL of rows
  0..3 (the strip at (0, 0)), where the Bohrium rule replaces the 8 diagonal
  elements.  The accelerations differ; the one built here is the second."""
  from nbody_ref import nbody_ref, unit_galaxy
  n, G = 8, 1.0
  x, y, z, m = unit_galaxy(n, np.float64, seed=1)
  strips = [(0, 4), (4, 8)]

  def per_tile(a, scalar):  # the reference's live rule, tile by tile
    out = a.copy()
    for lo, hi in strips:
      if lo == 0:  # ul = (lo, 0): on the diagonal only for the first strip
        out[lo:hi, :] = scalar
    return out

  def diagonal_only(a, scalar):
    out = a.copy()
    out[np.arange(n), np.arange(n)] = scalar
    return out

  def move_sums(set_diagonal):  # the reference's move(), typed out
    d = [-(p[None, :] - p[:, None]) for p in (x, y, z)]
    r = set_diagonal(np.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2), 1.0)
    mask = r < 1.0
    r = r * ~mask + 1.0 * mask
    return np.stack([set_diagonal(G * m[:, None] * dc / r ** 3, 0.0).sum(axis=0) for dc in d])

  live, intended = move_sums(per_tile), move_sums(diagonal_only)
  assert not np.allclose(live, intended, rtol=1e-3)
  # the live rule drops the pull of bodies 0..3 altogether
  half, _S = nbody_ref(x[4:], y[4:], z[4:], m[4:], G, 1.0, targets=(x, y, z))
  np.testing.assert_allclose(live, half, rtol=1e-12)
  want, S = nbody_ref(x, y, z, m, G, 1.0)
  assert np.all(np.abs(intended - want) <= 1e-14 * S)


# ------------------------------------------------------------- expr layer
def _bodies(dtype=np.float64, n=N, seed=5):
  r = np.random.RandomState(seed)
  return tuple((4.0 * r.randn(n)).astype(dtype) for _ in range(3)) + ((1.0 + r.rand(n)).astype(dtype),)


@pytest.mark.parametrize('W', [1, 2, 3])
@pytest.mark.parametrize('dtype', [np.float32, np.float64])
def test_nbody_every_layout(nbody_ctx, W, dtype):
  import torch
  be = nbody_ctx(W)
  from spartan_amd import expr
  from spartan_amd.array import distarray
  from nbody_ref import nbody_ref
  x, y, z, m = _bodies(dtype)
  want = nbody_ref(x, y, z, m, 0.7, 1.5)[0].astype(dtype)
  for hint in [(N,), (4,), (3,), (7,), 'replicated', 'host']:
    if hint == 'replicated':
      ops = [expr.lazify(distarray.ReplicatedArray(torch.as_tensor(a.copy()))) for a in (x, y, z, m)]
    elif hint == 'host':
      ops = [x, y, z, m]
    else:  # y, z and m tiled differently from x: another cut, one tile, a host array
      ops = [expr.lazify(expr.from_numpy(x, tile_hint=hint).force()),
             expr.lazify(expr.from_numpy(y, tile_hint=(5,)).force()),
             expr.lazify(expr.from_numpy(z, tile_hint=(N,)).force()), m]
    del be.calls[:], be.nbody_calls[:]
    parts = expr.nbody_accel(*ops, G=0.7, rmin=1.5)
    assert len(parts) == 3 and all(p.shape == (N,) and p.dtype == np.dtype(dtype) for p in parts)
    assert 'nbody_accel' not in be.calls  # lazy
    got_y = parts[1].glom()
    if isinstance(hint, tuple):
      cuts = sorted((e.ul[0], e.lr[0]) for e in ops[0].val.tiles)
      if hint in ((4,), (3,), (7,)):
        assert len(cuts) > 1 and len({hi - lo for lo, hi in cuts}) > 1  # an uneven cut
      assert sorted(be.nbody_calls) == sorted((hi - lo, N) for lo, hi in cuts), hint  # one launch per target slab
      for p in parts:
        assert sorted((e.ul[0], e.lr[0]) for e in p.force().tiles) == cuts, hint  # tiled at x's row cuts
    elif hint == 'replicated':
      assert be.nbody_calls == [(N, N)]
      assert isinstance(parts[0].force(), distarray.ReplicatedArray)
    else:  # a host array is distributed by the default tiling first
      assert be.calls.count('nbody_accel') >= 1
    launches = be.calls.count('nbody_accel')
    got = (parts[0].glom(), got_y, parts[2].glom())
    assert be.calls.count('nbody_accel') == launches, hint  # the triple evaluated once
    for c in range(3):  # equal to the single-tile answer, bit for bit
      assert got[c].dtype == np.dtype(dtype) and np.array_equal(got[c], want[c]), (hint, c)


def test_refusals(nbody_ctx):
  nbody_ctx(1)
  import scipy.sparse as sp
  from spartan_amd import expr
  x, y, z, m = _bodies()
  with pytest.raises(ValueError, match='1-d'):
    expr.nbody_accel(x.reshape(2, 5), y, z, m)
  with pytest.raises(ValueError, match='1-d'):
    expr.nbody_accel(x, y, z, m.reshape(N, 1))
  with pytest.raises(ValueError, match='one length'):
    expr.nbody_accel(x, y[:-1], z, m)
  with pytest.raises(ValueError, match='one length'):
    expr.nbody_accel(x, y, z, m[:3])
  with pytest.raises(ValueError, match='one dtype.*astype'):
    expr.nbody_accel(x, y.astype(np.float32), z, m)
  with pytest.raises(ValueError, match='astype'):
    expr.nbody_accel(*(a.astype(np.int64) for a in (x, y, z, m)))
  with pytest.raises(ValueError, match='astype'):
    expr.nbody_accel(x, y, z, np.arange(N, dtype=np.int32))
  for k in range(4):
    ops = [x, y, z, m]
    ops[k] = sp.csr_matrix(ops[k].reshape(1, N))
    with pytest.raises(TypeError, match=r'todense\(\)'):
      expr.nbody_accel(*ops)
  for bad in (float('nan'), float('inf')):
    with pytest.raises(ValueError, match='G = '):
      expr.nbody_accel(x, y, z, m, G=bad)
  for bad in (-1.0, float('nan'), float('inf')):
    with pytest.raises(ValueError, match='rmin'):
      expr.nbody_accel(x, y, z, m, rmin=bad)


# ------------------------------------------------------------------ driver
def test_random_galaxy_has_the_reference_keys_dtypes_and_ranges(nbody_ctx):
  nbody_ctx(2)
  from spartan_amd.examples import nbody
  assert (nbody.G, nbody.dt, nbody.r_ly, nbody.m_sol) == (6.67384e-11, 60 * 60 * 24 * 365.25, 9.4607e15, 1.9891e30)
  g = nbody.random_galaxy(200)
  assert sorted(g) == ['m', 'vx', 'vy', 'vz', 'x', 'y', 'z']
  vals = {k: v.glom() for k, v in g.items()}
  assert all(v.shape == (200,) and v.dtype == np.float64 for v in vals.values())
  assert np.all(vals['m'] >= nbody.m_sol) and np.all(vals['m'] < 1.1 * nbody.m_sol * (1 + 1e-15))
  for k in 'xyz':
    assert np.all(np.abs(vals[k]) <= nbody.r_ly / 200) and vals[k].std() > nbody.r_ly / 1000
    assert np.array_equal(vals['v' + k], np.zeros(200))
  assert not np.array_equal(vals['x'], vals['y'])


@pytest.mark.parametrize('W', [1, 3])
def test_driver_against_numpy_loop(nbody_ctx, W):
  be = nbody_ctx(W)
  from spartan_amd import expr
  from spartan_amd.examples import nbody
  from spartan_amd.expr import base
  from nbody_ref import nbody_loop, si_galaxy
  n = 33
  x, y, z, m = si_galaxy(n, np.float64)
  host = {'x': x, 'y': y, 'z': z, 'm': m, 'vx': np.zeros(n), 'vy': np.zeros(n), 'vz': np.zeros(n)}
  want = nbody_loop(host, nbody.G, 1.0, nbody.dt, 3)
  galaxy = {k: expr.from_numpy(v, tile_hint=(13,)) for k, v in host.items()}
  for step in range(3):
    slabs = len(expr.as_array(galaxy['x']).force().tiles)
    assert slabs == (3 if step == 0 else slabs)
    del be.calls[:]
    nbody.move(galaxy, nbody.dt)
    assert be.calls.count('nbody_accel') == 1 * slabs  # one launch per target slab a step
    for k in ('vx', 'vy', 'vz', 'x', 'y', 'z'):  # the state is arrays again, not this step's graph
      assert isinstance(galaxy[k], base.Val) and galaxy[k].val is not None
  del be.calls[:]
  got = {k: v.glom() for k, v in galaxy.items()}
  assert 'nbody_accel' not in be.calls  # nothing was left to evaluate
  for k in ('x', 'y', 'z', 'vx', 'vy', 'vz'):
    err = np.abs(got[k] - want[k]).max() / np.abs(want[k]).max()
    assert err <= 1e-12, (k, err)
  assert np.abs(want['vx']).max() > 0 and not np.array_equal(want['x'], x)
  # simulate() is timesteps moves of the module's dt
  again = {k: expr.from_numpy(v, tile_hint=(13,)) for k, v in host.items()}
  nbody.simulate(again, 3)
  assert all(np.array_equal(again[k].glom(), got[k]) for k in got)


# ------------------------------------------------------ the C ABI, no GPU
def _lib():
  import torch  # noqa: F401  (torch's HIP runtime first)
  from spartan_amd import binding
  return binding.load_library(), binding


@needs_lib
def test_plan_answers_without_gpu():
  lib, binding = _lib()
  for dtype in (np.float32, np.float64):
    tpb = binding.nbody_plan(dtype, 1, 1)[0]
    assert tpb >= 64 and tpb % 64 == 0
    for n in (0, 1, 257, 2051, 1 << 13, 1 << 17, 1 << 22):
      t, splits, nbytes = binding.nbody_plan(dtype, n, n)
      assert t == tpb and splits >= 1 and nbytes >= 0
      assert (nbytes == 0) == (splits == 1 or n == 0)
      if splits > 1:
        assert nbytes >= splits * 3 * n * 8  # float64 partials per split, component and target
    assert binding.nbody_plan(dtype, 0, 100) == (tpb, 1, 0) and binding.nbody_plan(dtype, 100, 0) == (tpb, 1, 0)
    # few targets against many sources are split; targets that fill the chip are not
    assert binding.nbody_plan(dtype, tpb, 1 << 17)[1] > 1
    assert binding.nbody_plan(dtype, 1 << 22, 1 << 17)[1] == 1
    # forced splits are taken as they are, and the workspace is monotone in them
    sizes = [binding.nbody_plan(dtype, 257, 257, s) for s in (1, 2, 3, 7, 64)]
    assert [s[1] for s in sizes] == [1, 2, 3, 7, 64]
    assert all(a[2] <= b[2] for a, b in zip(sizes, sizes[1:])) and sizes[0][2] == 0 < sizes[1][2]
    with pytest.raises(RuntimeError, match='splits'):
      binding.nbody_plan(dtype, 257, 257, 1 << 20)
    with pytest.raises(RuntimeError, match='splits'):
      binding.nbody_plan(dtype, 257, 257, -1)
  with pytest.raises(TypeError, match='float32 / float64'):
    binding.nbody_plan(np.int32, 1, 1)
  for bad in ((-1, 1), (1, -1)):
    with pytest.raises(ValueError, match='negative size'):
      binding.nbody_plan(np.float32, *bad)
  # the library's own answers to what the wrapper refuses first
  t, s, b = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_size_t(0)
  args = (ctypes.byref(t), ctypes.byref(s), ctypes.byref(b))
  assert lib.spx_nbody_plan(binding.SPX_I64, 1, 1, *args) == -3 and 'float32 / float64' in lib.spx_last_error().decode()
  assert lib.spx_nbody_plan(9, 1, 1, *args) == -1 and 'bad dtype' in lib.spx_last_error().decode()
  assert lib.spx_nbody_plan(binding.SPX_F32, -1, 1, *args) == -1 and 'negative size' in lib.spx_last_error().decode()
  assert lib.spx_nbody_plan(binding.SPX_F64, 1, -5, *args) == -1 and 'negative size' in lib.spx_last_error().decode()
  assert lib.spx_nbody_plan(binding.SPX_F64, 5, 5, None, None, None) == 0
  # sizes past the grid and past any index arithmetic are refused, not wrapped
  assert lib.spx_nbody_plan(binding.SPX_F64, 1, 2 ** 63 - 1, *args) == -3 and 'n_src' in lib.spx_last_error().decode()
  assert lib.spx_nbody_plan(binding.SPX_F64, 2 ** 63 - 1, 1, *args) == -3 and 'n_tgt' in lib.spx_last_error().decode()


@needs_lib
def test_argument_checks_without_gpu():
  lib, binding = _lib()
  F32, I64, EINVAL, ENOTSUP = binding.SPX_F32, binding.SPX_I64, -1, -3
  p = ctypes.c_void_p(4096)  # never dereferenced: every case fails its checks before any device work
  nul = ctypes.c_void_p(0)

  def accel(dtype=F32, n_tgt=5, tgt=p, n_src=7, src=p, sm=p, G=1.0, rmin=1.0, out=p, splits=1, ws=nul, nws=0):
    return lib.spx_nbody_accel(dtype, n_tgt, tgt, tgt, tgt, n_src, src, src, src, sm, G, rmin, out, out, out, splits,
                               ws, ctypes.c_size_t(nws), nul)

  def err():
    return lib.spx_last_error().decode()

  assert accel(dtype=I64) == ENOTSUP and 'float32 / float64' in err()
  assert accel(dtype=9) == EINVAL and 'bad dtype' in err()
  assert accel(n_tgt=-1) == EINVAL and 'negative size' in err()
  assert accel(n_src=-1) == EINVAL and 'negative size' in err()
  for bad in (float('nan'), float('inf')):
    assert accel(G=bad) == EINVAL and 'G = ' in err()
  for bad in (-1.0, float('nan'), float('inf')):
    assert accel(rmin=bad) == EINVAL and 'rmin' in err()
  assert accel(tgt=nul) == EINVAL and 'null pointer' in err()
  assert accel(out=nul) == EINVAL and 'null pointer' in err()
  assert accel(src=nul) == EINVAL and 'null pointer' in err()
  assert accel(sm=nul) == EINVAL and 'null pointer' in err()
  assert accel(splits=-1) == EINVAL and 'splits' in err()
  assert accel(splits=1 << 20) == EINVAL and 'splits' in err()
  # a forced split above what the workspace holds
  need = binding.nbody_plan(np.float32, 5, 7, 3)[2]
  assert need > 0
  assert accel(splits=3, ws=nul, nws=0) == EINVAL and 'workspace' in err()
  assert accel(splits=3, ws=p, nws=need - 1) == EINVAL and 'workspace' in err()
  assert accel(splits=3, ws=ctypes.c_void_p(4097), nws=need) == EINVAL and 'aligned' in err()
  # no targets: nothing is looked at, nothing is launched
  assert accel(n_tgt=0, tgt=nul, src=nul, sm=nul, out=nul) == 0


@needs_lib
def test_backend_wrapper_checks_without_gpu():
  """HipBackend.nbody_accel refuses what the kernel does not serve before any call."""
  import torch
  from spartan_amd import backend
  be = backend.HipBackend.__new__(backend.HipBackend)
  be._nbody_ws = {}
  v = torch.zeros((5,), dtype=torch.float32)
  s = torch.zeros((7,), dtype=torch.float32)

  def call(tx=v, ty=v, tz=v, sx=s, sy=s, sz=s, sm=s, G=1.0, rmin=1.0, splits=None):
    return be.nbody_accel(tx, ty, tz, sx, sy, sz, sm, G, rmin, splits)

  with pytest.raises(ValueError, match='1-d'):
    call(tx=torch.zeros((5, 1), dtype=torch.float32))
  with pytest.raises(ValueError, match='contiguous'):
    call(sm=torch.zeros((14,), dtype=torch.float32)[::2])
  with pytest.raises(ValueError, match='float32 / float64'):
    call(tx=v.to(torch.int64))
  with pytest.raises(ValueError, match='one dtype'):
    call(sz=s.to(torch.float64))
  with pytest.raises(ValueError, match='targets have unequal lengths'):
    call(ty=s)
  with pytest.raises(ValueError, match='sources have unequal lengths'):
    call(sm=v)
  with pytest.raises(ValueError, match='G = '):
    call(G=float('inf'))
  with pytest.raises(ValueError, match='rmin'):
    call(rmin=-0.5)
  with pytest.raises(ValueError, match='splits'):
    call(splits=-2)
  empty = torch.zeros((0,), dtype=torch.float32)
  out = call(tx=empty, ty=empty, tz=empty)  # no targets: no call into the library
  assert len(out) == 3 and all(t.shape == (0,) and t.dtype == torch.float32 for t in out)
