"""The yardstick and the inputs of the n-body tests, and the
CPU test double's ``nbody_accel``.

``nbody_ref`` evaluates, in NumPy float64 and LITERALLY as the formula reads,

    d_ij = p_i - p_j,  r_ij = sqrt(dx^2 + dy^2 + dz^2),  r_ij = rmin where r_ij < rmin,
    a_j  = sum_i G m_i d_ij / r_ij^3

chunked over the targets so that no (chunk, n) block is larger than a few MB.
Beside the three sums it returns ``S = sum_i |term_i|`` per target and
component: the accelerations are signed sums with cancellation, so errors are
measured against S, not against the result.
"""
import numpy as np
import torch

from fake_backend import FakeBackend

TOL = {np.dtype(np.float32): 1e-5, np.dtype(np.float64): 1e-12}
CHUNK_BYTES = 4 << 20


def _np(t):
  return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def nbody_ref(x, y, z, m, G, rmin, targets=None):
  """(a, S): float64 (3, n_tgt) accelerations and sums of the terms' magnitudes
  of the targets (default: the bodies themselves) under the sources x, y, z, m
  as stored (any float dtype, widened to float64)."""
  sx, sy, sz, sm = (np.asarray(a, np.float64) for a in (x, y, z, m))
  tx, ty, tz = (sx, sy, sz) if targets is None else (np.asarray(a, np.float64) for a in targets)
  n_tgt, n_src = tx.shape[0], sx.shape[0]
  a = np.zeros((3, n_tgt))
  S = np.zeros((3, n_tgt))
  chunk = max(1, CHUNK_BYTES // (8 * max(n_src, 1)))
  with np.errstate(invalid='ignore', divide='ignore'):
    for lo in range(0, n_tgt, chunk):
      hi = min(lo + chunk, n_tgt)
      # (chunk, n_src): target j down, source i across, so a target's sum is one row's and does not depend on the chunk
      d = [s[None, :] - t[lo:hi, None] for s, t in ((sx, tx), (sy, ty), (sz, tz))]
      r = np.sqrt(d[0] ** 2 + d[1] ** 2 + d[2] ** 2)
      r = np.where(r < rmin, rmin, r)  # (false for NaN: NaN stays)
      r3 = r ** 3
      for c in range(3):
        f = G * sm[None, :] * d[c] / r3
        a[c, lo:hi] = f.sum(axis=1)
        S[c, lo:hi] = np.abs(f).sum(axis=1)
  return a, S


def unit_galaxy(n, dtype, seed=3):
  """(x, y, z, m) on a unit scale: positions uniform in [-50, 50]^3, masses in
  [1, 2]; with rmin = 1 a few percent of the bodies have a neighbour inside the
  clamp from a few hundred bodies on."""
  r = np.random.RandomState(seed)
  x, y, z = (r.uniform(-50.0, 50.0, n).astype(dtype) for _ in range(3))
  return x, y, z, r.uniform(1.0, 2.0, n).astype(dtype)


def si_galaxy(n, dtype, seed=4):
  """(x, y, z, m) with the value ranges of the driver's ``random_galaxy`` in SI
  units: masses of 1 to 1.1 suns (2e30 kg), positions in a cube of a hundredth
  of a light year (9.5e13 m)."""
  r = np.random.RandomState(seed)
  m_sol, r_ly = 1.9891e30, 9.4607e15
  x, y, z = (((r.rand(n) - 0.5) * (r_ly / 100)).astype(dtype) for _ in range(3))
  return x, y, z, ((r.rand(n) + 10.0) * (m_sol / 10)).astype(dtype)


def clamped_pairs(x, y, z, rmin):
  """The number of ordered pairs i != j closer than rmin."""
  p = np.stack([np.asarray(a, np.float64) for a in (x, y, z)], axis=1)
  n, count = p.shape[0], 0
  for lo in range(0, n, 512):
    d = np.sqrt(((p[lo:lo + 512, None, :] - p[None, :, :]) ** 2).sum(axis=2))
    count += int((d < rmin).sum()) - min(512, n - lo)
  return count


def nbody_loop(galaxy, G, rmin, dt, steps):
  """The NumPy model of the driver: ``steps`` of v += dt a, then x += dt v, on
  a dict of float64 host arrays (not modified); returns the new dict."""
  g = {k: np.array(v, np.float64) for k, v in galaxy.items()}
  for _ in range(steps):
    a, _S = nbody_ref(g['x'], g['y'], g['z'], g['m'], G, rmin)
    for c, k in enumerate('xyz'):
      g['v' + k] = g['v' + k] + dt * a[c]
    for k in 'xyz':
      g[k] = g[k] + dt * g['v' + k]
  return g


# -------------------------------------------------------------- test double
class NbodyFakeBackend(FakeBackend):
  """The CPU test double + ``nbody_accel`` by the yardstick; ``nbody_calls``
  records (n_tgt, n_src) of every call."""

  def __init__(self):
    FakeBackend.__init__(self)
    self.nbody_calls = []

  def nbody_accel(self, tx, ty, tz, sx, sy, sz, sm, G, rmin, splits=None):
    arrs = [_np(t) for t in (tx, ty, tz, sx, sy, sz, sm)]
    dt = arrs[0].dtype
    assert dt in (np.float32, np.float64) and all(a.ndim == 1 and a.dtype == dt for a in arrs)
    assert len({a.shape for a in arrs[:3]}) == 1 and len({a.shape for a in arrs[3:]}) == 1
    a, _S = nbody_ref(*arrs[3:], G, rmin, targets=arrs[:3])
    self.calls.append('nbody_accel')
    self.nbody_calls.append((arrs[0].shape[0], arrs[3].shape[0]))
    return tuple(torch.as_tensor(a[c].astype(dt)) for c in range(3))
