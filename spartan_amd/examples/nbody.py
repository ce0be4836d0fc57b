"""The reference's n-body driver (spartan/examples/nbody.py, after the Bohrium
example it cites) on the direct-sum kernel (``expr.nbody_accel``, DESIGN.md
3.26).

The reference's ``move`` builds about a dozen (n, n) float64 arrays a time
step.  Here a step is one all-pairs kernel launch per slab of bodies, which
reads the positions and masses and writes the three acceleration vectors, and
six ordinary maps for ``v += dt a`` and ``x += dt v``, in the reference's order.

Divergences from the reference, kept on purpose:

  * THE DIAGONAL RULE.  The reference's ``_set_diagonal_mapper`` returns the
    scalar IN PLACE OF THE WHOLE TILE whenever the tile's upper-left corner lies
    on the diagonal.  With its default row-strip tiling the first strip starts
    at (0, 0), so ``set_diagonal(r, 1.0)`` replaces the entire first strip of
    the distances by 1.0 and ``set_diagonal(f, 0.0)`` the entire first strip of
    the forces by 0.0: the first n / workers bodies exert nothing on anybody.
    The rule built here is the one of the Bohrium original the reference's
    docstring cites: only the diagonal ELEMENTS are replaced (r_jj = 1, f_jj =
    0).  With the clamp ``r = rmin where r < rmin`` that needs no special case
    at all: for i = j, d = 0 and r = rmin, so the term is exactly 0;
  * the six state arrays are forced at the end of every step (the reference's
    commented-out ``eager`` calls), so the expression graph does not grow
    across steps.

Not built: Barnes-Hut, FMM or any other sub-quadratic method; periodic
boundaries; the potential energy; targets other than the bodies themselves;
a galaxy too large for one GPU to hold all positions and masses.
"""
import numpy as np

from .. import expr

G = 6.67384e-11           # m/(kg*(s^2))
dt = 60 * 60 * 24 * 365.25  # Years in seconds
r_ly = 9.4607e15          # Lightyear in m
m_sol = 1.9891e30         # Solar mass in kg

_STATE = ('vx', 'vy', 'vz', 'x', 'y', 'z')


def random_galaxy(n):
  """A galaxy of ``n`` random bodies, all standing still: a dict of float64
  (n,) expressions ``m`` (1 to 1.1 solar masses), ``x, y, z`` (a cube of a
  hundredth of a light year) and ``vx, vy, vz`` (zeros)."""
  return {
      'm': (expr.rand(n) + 10.0) * (m_sol / 10),
      'x': (expr.rand(n) - 0.5) * (r_ly / 100),
      'y': (expr.rand(n) - 0.5) * (r_ly / 100),
      'z': (expr.rand(n) - 0.5) * (r_ly / 100),
      'vx': expr.zeros((n,)),
      'vy': expr.zeros((n,)),
      'vz': expr.zeros((n,)),
  }


def move(galaxy, dt):
  """Move the bodies one step of ``dt`` seconds, in place in the dict: first
  the accelerations change the velocities, then the velocities the positions."""
  ax, ay, az = expr.nbody_accel(galaxy['x'], galaxy['y'], galaxy['z'], galaxy['m'], G=G, rmin=1.0)
  galaxy['vx'] = galaxy['vx'] + dt * ax
  galaxy['vy'] = galaxy['vy'] + dt * ay
  galaxy['vz'] = galaxy['vz'] + dt * az
  galaxy['x'] = galaxy['x'] + dt * galaxy['vx']
  galaxy['y'] = galaxy['y'] + dt * galaxy['vy']
  galaxy['z'] = galaxy['z'] + dt * galaxy['vz']
  for key in _STATE:  # evaluated now: the next step starts from arrays, not from this step's graph
    galaxy[key] = expr.lazify(expr.as_array(galaxy[key]).force())


def simulate(galaxy, timesteps):
  for _ in range(timesteps):
    move(galaxy, dt)
