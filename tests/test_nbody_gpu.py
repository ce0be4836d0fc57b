"""spx_nbody_accel, ``expr.nbody_accel`` and the n-body driver on a real MI355X
(DESIGN.md 3.26), at the sizes where the kernel can go wrong: one and two
bodies; one body less than, exactly and one more than a wave (64), a workgroup's
lanes (256), a workgroup's targets (tgt_per_block, from the plan) and a source
tile (TS, from the kernel's header); 1000 and 2051.  The plan cuts the sources
of every case above 128 bodies into ranges, so the partials and their ordered
sum are part of the plain parity cases too.

The yardstick is nbody_ref.nbody_ref -- the formula evaluated literally in
float64 on the same, already rounded, inputs.  The accelerations are signed
sums with cancellation, so the error is measured against S = sum_i |term_i| per
target and component: ``|a - a_ref| <= tol * S`` element-wise with the
project's parity tolerances, 1e-12 (float64) and 1e-5 (float32).  Both sides of
a float64 case are within n 2^-53 = 2.3e-13 of exact at n <= 2051.  A single
sequential float32 sum of 2051 terms could be off by n 2^-24 = 1.2e-4: the
kernel sums at most 32 terms in float32 before it adds them to a float64
accumulator, 32 * 2^-24 = 1.9e-6 plus about 6e-7 for the rounding of a term.
"""
import functools
import os
import re

import numpy as np
import pytest

from nbody_ref import TOL, clamped_pairs, nbody_loop, nbody_ref, si_galaxy, unit_galaxy

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
HEADER = os.path.join(os.path.dirname(HERE), 'spartan_amd', 'csrc', 'nbody_kernels.h')
DTYPES = [np.float32, np.float64]


SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 2051]


def _edges(dtype):
  """One value on each side of tgt_per_block (the plan's) and of the source tile (the header's)."""
  from spartan_amd import binding
  tpb = binding.nbody_plan(dtype, 1, 1)[0]
  ts = int(re.search(r'constexpr int TS = (\d+);', open(HEADER).read()).group(1))
  return sorted({tpb - 1, tpb + 1, ts - 1, ts + 1} - set(SIZES))


def _dev(a):
  import torch
  return torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared inputs are read-only)


def _host(ts):
  return np.stack([t.cpu().numpy() for t in ts])


@functools.lru_cache(maxsize=None)
def _case(kind, n, dtype):
  """(x, y, z, m, G, rmin, a_ref, S) of one case, computed once and shared (never written)."""
  if kind == 'unit':
    x, y, z, m = unit_galaxy(n, dtype)
    if n >= 2:  # a pair of distinct bodies inside the clamp in every case
      x[1], y[1], z[1] = x[0] + dtype(0.3), y[0] + dtype(0.2), z[0] - dtype(0.1)
    G, rmin = 1.0, 1.0
  else:
    x, y, z, m = si_galaxy(n, dtype)
    G, rmin = 6.67384e-11, 1.0
  a, S = nbody_ref(x, y, z, m, G, rmin)
  for arr in (x, y, z, m, a, S):
    arr.setflags(write=False)
  return x, y, z, m, G, rmin, a, S


def _accel(x, y, z, m, G, rmin, targets=None, splits=None):
  from spartan_amd import backend
  s = [_dev(v) for v in (x, y, z, m)]
  t = s[:3] if targets is None else [_dev(v) for v in targets]
  return _host(backend.get().nbody_accel(t[0], t[1], t[2], s[0], s[1], s[2], s[3], G, rmin, splits))


def _check(what, dtype, got, a, S):
  tol = TOL[np.dtype(dtype)]
  assert got.dtype == np.dtype(dtype) and got.shape == a.shape, what
  err = np.abs(got.astype(np.float64) - a)
  with np.errstate(invalid='ignore', divide='ignore'):
    worst = float(np.max(np.where(S > 0, err / S, np.where(err > 0, np.inf, 0.0)))) if err.size else 0.0
  print('%s: max |a - a_ref| / S = %.3g (tolerance %.3g)' % (what, worst, tol))
  assert np.all(np.isfinite(got)), what
  assert np.all(err <= tol * S), what


# ------------------------------------------------------------ spx_nbody_accel
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n', SIZES)
def test_unit_scale_against_yardstick(gpu_ctx, n, dtype):
  x, y, z, m, G, rmin, a, S = _case('unit', n, dtype)
  if n >= 2:
    assert clamped_pairs(x, y, z, rmin) >= 2  # (ordered pairs: the planted one, both ways)
  _check('unit n=%d %s' % (n, np.dtype(dtype)), dtype, _accel(x, y, z, m, G, rmin), a, S)


@pytest.mark.parametrize('dtype', DTYPES)
def test_block_and_tile_edges_against_yardstick(gpu_ctx, dtype):
  edges = _edges(dtype)
  assert edges and min(edges) > 2
  for n in edges:
    x, y, z, m, G, rmin, a, S = _case('unit', n, dtype)
    _check('unit n=%d %s' % (n, np.dtype(dtype)), dtype, _accel(x, y, z, m, G, rmin), a, S)


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('n', [257, 2051])
def test_reference_scale_against_yardstick(gpu_ctx, n, dtype):
  """``random_galaxy``'s values in SI units: G m near 1e20, r near 1e14, r^3 near
  1e42 -- beyond float32, which the kernel never forms."""
  x, y, z, m, G, rmin, a, S = _case('si', n, dtype)
  assert float(np.abs(x).max()) ** 3 > 1e38 and np.all(S[:, 0] > 0)
  _check('SI n=%d %s' % (n, np.dtype(dtype)), dtype, _accel(x, y, z, m, G, rmin), a, S)


@pytest.mark.parametrize('dtype', DTYPES)
def test_rectangular_and_empty_calls(gpu_ctx, dtype):
  import torch
  from spartan_amd import backend
  x, y, z, m, G, rmin, _a, _S = _case('unit', 1000, dtype)
  for tgt, src in ((slice(0, 100), slice(0, 1000)), (slice(0, 1000), slice(900, 1000)), (slice(37, 38), slice(0, 999))):
    t = (x[tgt], y[tgt], z[tgt])
    a, S = nbody_ref(x[src], y[src], z[src], m[src], G, rmin, targets=t)
    got = _accel(x[src], y[src], z[src], m[src], G, rmin, targets=t)
    _check('%s targets, %s sources, %s' % (tgt, src, np.dtype(dtype)), dtype, got, a, S)
  be = backend.get()
  full = [_dev(v) for v in (x, y, z, m)]
  none = [torch.empty((0,), dtype=full[0].dtype, device='cuda') for _ in range(4)]
  out = be.nbody_accel(*none[:3], *full, G, rmin)
  assert all(t.shape == (0,) and t.dtype == full[0].dtype for t in out)
  out = _host(be.nbody_accel(*full[:3], *none, G, rmin))
  assert out.shape == (3, 1000) and out.dtype == np.dtype(dtype) and np.array_equal(out, np.zeros((3, 1000)))


@pytest.mark.parametrize('dtype', DTYPES)
def test_forced_splits(gpu_ctx, dtype):
  """The same inputs at n = 257 in 1, 2, 3 and 7 source ranges: each within
  tolerance, each bitwise equal to itself on a second call."""
  x, y, z, m, G, rmin, a, S = _case('unit', 257, dtype)
  for splits in (1, 2, 3, 7):
    got = _accel(x, y, z, m, G, rmin, splits=splits)
    _check('n=257 splits=%d %s' % (splits, np.dtype(dtype)), dtype, got, a, S)
    assert _accel(x, y, z, m, G, rmin, splits=splits).tobytes() == got.tobytes(), splits


@pytest.mark.parametrize('dtype', DTYPES)
def test_special_values(gpu_ctx, dtype):
  one = dtype(1.0)
  # two bodies at one position: exactly nothing on each other (and no NaN from 0 / 0)
  got = _accel(*(np.array([v, v], dtype) for v in (1.5, -2.0, 3.25, 4.0)), 2.0, 1.0)
  assert np.array_equal(got, np.zeros((3, 2))) and got.dtype == np.dtype(dtype)
  # ... and a third body pulls both of them alike
  x, y, z, m = (np.array(v, dtype) for v in ([1, 1, 9], [2, 2, 2], [3, 3, 3], [5, 7, 11]))
  got = _accel(x, y, z, m, 1.0, 1.0)
  assert got[0, 0] == got[0, 1] and got[0, 0] > 0 and np.array_equal(got[1:], np.zeros((2, 3)))
  # one NaN position: all 3 n outputs are NaN (n = 1000: several source ranges)
  x, y, z, m, G, rmin, _a, _S = _case('unit', 1000, dtype)
  bad = np.array(x)
  bad[613] = np.nan
  assert np.all(np.isnan(_accel(bad, y, z, m, G, rmin)))
  # a body without mass feels the others and exerts nothing: where it stands changes nobody else's bits
  x, y, z, m, G, rmin, _a, _S = _case('unit', 300, dtype)
  m0 = np.array(m)
  m0[17] = 0
  a, S = nbody_ref(x, y, z, m0, G, rmin)
  got = _accel(x, y, z, m0, G, rmin)
  _check('m = 0 %s' % np.dtype(dtype), dtype, got, a, S)
  assert np.all(got[:, 17] != 0)
  moved = [np.array(v) for v in (x, y, z)]
  for v in moved:
    v[17] += one
  others = np.arange(300) != 17
  assert np.array_equal(_accel(*moved, m0, G, rmin)[:, others], got[:, others])


# ------------------------------------------------------------------ expr layer
@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('W', [1, 2, 3])
def test_expr_layouts_on_the_device(gpu_workers, W, dtype):
  gpu_workers(W)
  from spartan_amd import expr
  x, y, z, m, G, rmin, a, S = _case('unit', 1000, dtype)
  for hint in ((1000,), (300,), (129,)):  # one slab; 300 300 300 100; 129 x 7 and 97
    ops = [expr.from_numpy(x, tile_hint=hint), expr.from_numpy(y, tile_hint=(500,)), expr.from_numpy(z), m]
    parts = expr.nbody_accel(*ops, G=G, rmin=rmin)
    got = np.stack([p.glom() for p in parts])
    _check('workers %d hint %s %s' % (W, hint, np.dtype(dtype)), dtype, got, a, S)
    cuts = sorted((e.ul[0], e.lr[0]) for e in ops[0].force().tiles)
    assert sorted((e.ul[0], e.lr[0]) for e in parts[2].force().tiles) == cuts


@pytest.mark.parametrize('dtype', DTYPES)
def test_two_evaluations_are_bitwise_equal(gpu_workers, dtype):
  gpu_workers(2)
  from spartan_amd import expr
  x, y, z, m, G, rmin, _a, _S = _case('unit', 2051, dtype)
  ops = [expr.lazify(expr.from_numpy(v, tile_hint=(700,)).force()) for v in (x, y, z, m)]
  first = np.stack([p.glom() for p in expr.nbody_accel(*ops, G=G, rmin=rmin)])
  again = np.stack([p.glom() for p in expr.nbody_accel(*ops, G=G, rmin=rmin)])
  assert first.tobytes() == again.tobytes()


# ---------------------------------------------------------------------- driver
@pytest.mark.parametrize('dtype', DTYPES)
def test_driver_on_the_device(gpu_workers, dtype):
  """Two steps of ``simulate`` on n = 300 against the NumPy loop.  The bound is
  the acceleration tolerance carried through the update, per element, with
  tau the parity tolerance, u the dtype's epsilon (each update is a multiply
  and an add; 4 u covers them and the rounding of dt), S_k the yardstick's S at
  step k and L_j = sum_i 4 G m_i / r_ij^3 the bound on how far a component of
  a_j moves per metre by which a separation vector is off (|grad (d_c / r^3)|
  <= 4 / r^3; a separation is off by at most 2 sqrt(3) times the largest
  coordinate error; no pair is near the clamp, which the test asserts):

    E_v1 = dt tau S_0 + 4 u |v_1|          E_x1 = dt E_v1 + 4 u |x_1|
    E_a1 = tau S_1 + L * 2 sqrt(3) max E_x1
    E_v2 = E_v1 + dt E_a1 + 4 u |v_2|      E_x2 = E_x1 + dt E_v2 + 4 u |x_2|
  """
  gpu_workers(2)
  from spartan_amd import expr
  from spartan_amd.examples import nbody
  n, tau, u = 300, TOL[np.dtype(dtype)], float(np.finfo(dtype).eps)
  x, y, z, m = si_galaxy(n, dtype)
  zero = np.zeros(n, dtype)
  host = {'x': x, 'y': y, 'z': z, 'm': m, 'vx': zero, 'vy': zero, 'vz': zero}
  dt, G = nbody.dt, nbody.G
  s1 = nbody_loop(host, G, 1.0, dt, 1)
  s2 = nbody_loop(host, G, 1.0, dt, 2)
  S0 = nbody_ref(x, y, z, m, G, 1.0)[1]
  S1 = nbody_ref(s1['x'], s1['y'], s1['z'], m, G, 1.0)[1]
  p = np.stack([s1['x'], s1['y'], s1['z']], axis=1)
  r = np.sqrt(((p[:, None, :] - p[None, :, :]) ** 2).sum(axis=2))
  np.fill_diagonal(r, np.inf)
  assert r.min() > 1e6  # metres: nowhere near rmin = 1
  L = (4.0 * G * np.asarray(m, np.float64)[None, :] / r ** 3).sum(axis=1)
  v1 = np.stack([s1['vx'], s1['vy'], s1['vz']])
  x1 = np.stack([s1['x'], s1['y'], s1['z']])
  v2 = np.stack([s2['vx'], s2['vy'], s2['vz']])
  x2 = np.stack([s2['x'], s2['y'], s2['z']])
  E_v1 = dt * tau * S0 + 4 * u * np.abs(v1)
  E_x1 = dt * E_v1 + 4 * u * np.abs(x1)
  E_a1 = tau * S1 + L[None, :] * 2.0 * np.sqrt(3.0) * E_x1.max()
  E_v2 = E_v1 + dt * E_a1 + 4 * u * np.abs(v2)
  E_x2 = E_x1 + dt * E_v2 + 4 * u * np.abs(x2)

  galaxy = {k: expr.from_numpy(v, tile_hint=(128,)) for k, v in host.items()}
  nbody.simulate(galaxy, 2)
  got = {k: v.glom() for k, v in galaxy.items()}
  for c, k in enumerate('xyz'):
    assert got[k].dtype == np.dtype(dtype) and got['v' + k].dtype == np.dtype(dtype)
    ev = np.abs(got['v' + k].astype(np.float64) - v2[c])
    ex = np.abs(got[k].astype(np.float64) - x2[c])
    print('driver %s %s: max |dv| / E_v2 = %.3g, max |dx| / E_x2 = %.3g'
          % (np.dtype(dtype), k, float((ev / E_v2[c]).max()), float((ex / E_x2[c]).max())))
    assert np.all(ev <= E_v2[c]) and np.all(ex <= E_x2[c])
  assert np.abs(v2).min() > 0 and not np.array_equal(x2, np.stack([x, y, z]).astype(np.float64))
