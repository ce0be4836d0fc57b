"""Shared by tests/test_eigh.py and tests/test_eigh_gpu.py: the data kinds, the
error ratios, the yardstick and the CPU test double of DESIGN.md 3.21.

With u the unit roundoff of the data's dtype, evaluated in np.longdouble:

  res  = max_j ||A v_j - w_j v_j||_2 / (u ||A||_F)   (a zero matrix must give an
         exactly zero residual),
  orth = ||V^T V - I||_2 / u,
  ev   = max_j |w_j - lam_(j)| / (u max |lam|)        where the spectrum lam is
         prescribed.

The yardstick, per (dtype, n), is the larger ratio over all data kinds of

  * ``jacobi_model``: a NumPy restatement, in the data's own dtype, of the
    method spx_syevj is specified to run (scaling by a power of two, the
    threshold tau = u ||A||_F / n, Rutishauser's rotation, round-robin sweeps).
    It is written from the specification, not from the kernel, and shares no
    code with it;
  * LAPACK: ``scipy.linalg.eigh(driver='evd')`` in the data's dtype
    (``np.linalg.eigh`` is not used: NumPy's float32 ``eigh`` may compute in
    double, which would understate what single precision can do).

A Jacobi method is inherently less orthogonal than a Householder-based one
(each column of V takes about sweeps * n rotations), so LAPACK alone is the
wrong yardstick.  A result passes within FACTOR = 4 x the yardstick: the
margin of qr_ref, for a different but equally valid order of rotations and
sums.

So that the yardstick cannot hide a broken model, an unconditional envelope
holds besides: orth <= 4 n sqrt(S) u with S the sweeps used (a random walk
over the S (n - 1) rounds, over n columns; the constant peaked at 1.66 for the
model over all kinds, n <= 128), and orth == 0 exactly when S == 0.
"""
import numpy as np
import torch

from fake_backend import _np
from linalg_ref import LD, LinalgFakeBackend, _wide, same_bits, unit_roundoff  # noqa: F401  (re-exported)

KINDS = ('gauss', 'tridiag', 'graded', 'posdef', 'pm', 'cluster', 'rankdef', 'diag', 'exchange', 'zero')
FACTOR = 4
SWEEP_MAX = 64


# ------------------------------------------------------------------- data
def _with_spectrum(lam, r):
  """Q diag(lam) Q^T in np.longdouble, Q the product of n random Householder
  reflectors, symmetrised."""
  n = lam.size
  M = np.diag(lam.astype(LD))
  for _ in range(n):
    v = r.standard_normal(n).astype(LD)
    v /= np.sqrt((v * v).sum())
    Mv = M.dot(v)
    vMv = v.dot(Mv)
    # H M H, H = I - 2 v v^T (M symmetric)
    M = M - 2 * np.outer(v, Mv) - 2 * np.outer(Mv, v) + 4 * vMv * np.outer(v, v)
    M = (M + M.T) / 2
  return M


def eigh_data(kind, n, dtype, seed=0):
  """(A, lam): a symmetric (n, n) matrix of ``dtype`` and its prescribed
  spectrum in ascending order (np.longdouble), or None.  kind:
    'gauss'     (G + G^T) / 2, G standard normal;
    'tridiag'   random symmetric tridiagonal (the Lanczos case);
    'graded'    D G D, G symmetrised Gaussian, D = logspace(0, -6 | -15)
                (float32 | float64);
    'posdef'    spectrum logspace(0, -5 | -13): positive definite, that cond;
    'pm'        lam and -lam both present, plus a zero for odd n;
    'cluster'   two thirds of the spectrum exactly 1, the rest within 1e-3;
    'rankdef'   half the spectrum exactly 0;
    'diag'      a diagonal matrix of small integers (exact in every dtype);
    'exchange'  ones on the anti-diagonal, zero diagonal;
    'zero'      all zeros."""
  dt = np.dtype(dtype)
  f32 = dt == np.float32
  r = np.random.RandomState(seed + 7919 * n + (0 if f32 else 13))
  lam = None
  if kind == 'gauss':
    G = r.standard_normal((n, n))
    A = (G + G.T) / 2
  elif kind == 'tridiag':
    A = np.diag(r.standard_normal(n))
    off = r.standard_normal(max(n - 1, 0))
    A += np.diag(off, 1) + np.diag(off, -1)
  elif kind == 'graded':
    G = r.standard_normal((n, n))
    d = np.logspace(0, -6 if f32 else -15, n)
    A = d[:, None] * ((G + G.T) / 2) * d[None, :]
  elif kind in ('posdef', 'pm', 'cluster', 'rankdef'):
    if kind == 'posdef':
      lam = np.logspace(0, -5 if f32 else -13, n)
    elif kind == 'pm':
      h = 1.0 + r.uniform(size=n // 2)
      lam = np.concatenate([h, -h, np.zeros(n % 2)])
    elif kind == 'cluster':
      k = (2 * n) // 3
      lam = np.concatenate([np.ones(k), 1.0 + 1e-3 * r.uniform(-1, 1, size=n - k)])
    else:
      lam = np.concatenate([np.zeros(n // 2), 1.0 + r.uniform(size=n - n // 2)])
    lam = np.sort(lam.astype(LD))
    A = _with_spectrum(lam, r)
  elif kind == 'diag':
    d = ((np.arange(n) * 5) % 11 - 4).astype(np.float64)
    A = np.diag(d)
    lam = np.sort(d.astype(LD))
  elif kind == 'exchange':
    A = np.fliplr(np.eye(n))
    A[np.arange(n), np.arange(n)] = 0.0
    lam = np.sort(np.concatenate([-np.ones(n // 2), np.zeros(n % 2), np.ones(n // 2)]).astype(LD))
  elif kind == 'zero':
    A = np.zeros((n, n))
    lam = np.zeros(n, LD)
  else:
    raise ValueError(kind)
  A = np.asarray(A).astype(dt)  # rounded once
  A = np.ascontiguousarray(np.tril(A) + np.tril(A, -1).T)  # exactly symmetric
  return A, lam


# ----------------------------------------------------------------- ratios
def eigh_ratios(A, w, V, lam=None):
  """(res, orth, ev) in units of u; ev is None without a prescribed spectrum."""
  dt = A.dtype
  _wide(dt)
  n = A.shape[0]
  assert w.shape == (n,) and V.shape == (n, n) and w.dtype == dt and V.dtype == dt
  assert np.all(np.isfinite(w)) and np.all(np.isfinite(V)), 'non-finite entries in the result'
  u = unit_roundoff(dt)
  a, wl, v = A.astype(LD), w.astype(LD), V.astype(LD)
  d = a.dot(v) - v * wl[None, :]
  rn = np.sqrt((d * d).sum(0))
  an = np.sqrt((a * a).sum())
  if an == 0:
    assert not np.any(rn != 0), 'a nonzero residual for the zero matrix'
    res = 0.0
  else:
    res = float(rn.max() / (u * an)) if n else 0.0
  e = v.T.dot(v) - np.eye(n, dtype=LD)
  scale = np.abs(e).max() if n else 0
  orth = 0.0
  if scale > 0:  # the 2-norm of the scaled matrix in double: 1e-16 relative, on a quantity of a few u
    orth = float(LD(np.linalg.norm((e / scale).astype(np.float64), 2)) * scale / u)
  ev = None
  if lam is not None:
    top = np.abs(lam).max() if n else 0
    diff = np.abs(wl - np.sort(lam.astype(LD)))
    if top == 0:
      assert not np.any(diff != 0), 'a nonzero eigenvalue for the zero spectrum'
      ev = 0.0
    else:
      ev = float(diff.max() / (u * top))
  return res, orth, ev


def envelope(n, sweeps, dtype=None):
  """The bound on orth, in units of u, for ``sweeps`` sweeps at size n."""
  return 4.0 * n * np.sqrt(float(sweeps))


# ------------------------------------------------------------ the ordering
def round_robin(m):
  """The m - 1 rounds of a tournament over m (even) indices: a list of rounds,
  each a list of m / 2 disjoint pairs (p < q); every pair occurs exactly once.
  (The circle method: index m - 1 stays, the others rotate.)"""
  assert m % 2 == 0 and m >= 2
  ring = list(range(m - 1))
  rounds = []
  for r in range(m - 1):
    rot = ring[r:] + ring[:r]
    pairs = [(min(m - 1, rot[0]), max(m - 1, rot[0]))]
    for k in range(1, m // 2):
      x, y = rot[k], rot[-k]
      pairs.append((min(x, y), max(x, y)))
    rounds.append(pairs)
  return rounds


def canonical(w, V):
  """(w, V) in the contract's form: ascending, stable; every column's entry of
  largest magnitude (the first on a tie) positive."""
  order = np.argsort(w, kind='stable')
  w, V = w[order], V[:, order].copy()
  for j in range(V.shape[1]):
    i = int(np.argmax(np.abs(V[:, j])))  # the first maximum
    if V[i, j] < 0:
      V[:, j] = -V[:, j]
  return np.ascontiguousarray(w), np.ascontiguousarray(V)


# --------------------------------------------------------------- the model
def jacobi_model(A, sweep_max=SWEEP_MAX):
  """(w, V, sweeps) of the symmetric ``A`` by the specified method, every
  operation in A's dtype (the norm of the threshold in double); sweeps == -1
  (and NaN results) where it does not converge or A is not finite."""
  dt = A.dtype
  T = dt.type
  n = A.shape[0]
  nan = (np.full(n, np.nan, dt), np.full((n, n), np.nan, dt), -1)
  if n == 0:
    return np.zeros(0, dt), np.zeros((0, 0), dt), 0
  big = np.abs(A).max()
  if not np.isfinite(big):
    return nan
  if big == 0:
    return np.zeros(n, dt), np.eye(n, dtype=dt), 0
  e = int(np.floor(np.log2(float(big))))
  while 2.0 ** e > big:
    e -= 1
  while 2.0 ** (e + 1) <= big:
    e += 1
  a = np.ldexp(A, -e).astype(dt)
  V = np.eye(n, dtype=dt)
  u = float(unit_roundoff(dt))
  tau = T(u * np.sqrt((a.astype(np.float64) ** 2).sum()) / n)
  if n == 1:
    return np.ldexp(np.diag(a), e).astype(dt), V, 0
  m = n + (n & 1)
  rounds = [(np.array([p for p, q in pairs if q < n]), np.array([q for p, q in pairs if q < n]))
            for pairs in round_robin(m)]
  one = T(1)
  sweeps = -1
  with np.errstate(all='ignore'):
    for sweep in range(sweep_max):
      rotated = False
      for P, Q in rounds:
        apq = a[P, Q]
        hit = np.abs(apq) > tau
        if not hit.any():
          continue
        rotated = True
        P, Q, apq = P[hit], Q[hit], apq[hit]
        app, aqq = a[P, P], a[Q, Q]
        theta = (aqq - app) / (T(2) * apq)
        t = one / (np.abs(theta) + np.sqrt(theta * theta + one))
        t = np.where(theta < 0, -t, t).astype(dt)
        c = (one / np.sqrt(t * t + one)).astype(dt)
        s = (t * c).astype(dt)
        for M in (a, V):
          xp, xq = M[:, P], M[:, Q]
          M[:, P] = c * xp - s * xq
          M[:, Q] = s * xp + c * xq
        xp, xq = a[P, :], a[Q, :]
        a[P, :] = c[:, None] * xp - s[:, None] * xq
        a[Q, :] = s[:, None] * xp + c[:, None] * xq
        a[P, P] = app - t * apq
        a[Q, Q] = aqq + t * apq
        a[P, Q] = 0
        a[Q, P] = 0
      if not rotated:
        sweeps = sweep + 1
        break
  if sweeps < 0:
    return nan
  w, V = canonical(np.ldexp(np.diag(a), e).astype(dt), V)
  return w, V, sweeps


def lapack_eigh(A):
  from scipy.linalg import eigh
  if A.shape[0] == 0:
    return np.zeros(0, A.dtype), np.zeros((0, 0), A.dtype)
  w, V = eigh(A, driver='evd', check_finite=False)
  assert w.dtype == A.dtype and V.dtype == A.dtype  # the data's own precision
  return w, V


# ------------------------------------------------------------ the yardstick
_YARD = {}
_MODEL = {}


def model_run(kind, n, dtype, seed=0):
  """(A, lam, (res, orth, ev), sweeps) of the model on one data kind (cached)."""
  key = (kind, n, np.dtype(dtype).str, seed)
  if key not in _MODEL:
    A, lam = eigh_data(kind, n, dtype, seed)
    w, V, sweeps = jacobi_model(A)
    assert sweeps >= 0, 'the model did not converge on %s' % (key,)
    _MODEL[key] = (eigh_ratios(A, w, V, lam), sweeps)
  return _MODEL[key]


def yardstick(dtype, n, seed=0):
  """(Y_res, Y_orth, Y_ev): the largest ratios of the model and of LAPACK over
  KINDS at (dtype, n)."""
  key = (np.dtype(dtype).str, n, seed)
  if key not in _YARD:
    y = [0.0, 0.0, 0.0]
    for kind in KINDS:
      A, lam = eigh_data(kind, n, dtype, seed)
      for ratios in (model_run(kind, n, dtype, seed)[0], eigh_ratios(A, *lapack_eigh(A), lam=lam)):
        for i, x in enumerate(ratios):
          if x is not None:
            y[i] = max(y[i], x)
    _YARD[key] = tuple(y)
  return _YARD[key]


def assert_ratios(A, w, V, lam, sweeps, yard, what):
  """The three ratios within FACTOR x the yardstick, and the envelope for the
  ``sweeps`` the solver reported (None: not known, no envelope); returns the
  ratios."""
  n = A.shape[0]
  res, orth, ev = eigh_ratios(A, w, V, lam)
  print('%s: res %.3g u (yardstick %.3g), orth %.3g u (yardstick %.3g, envelope %.3g), ev %s u (yardstick %.3g), '
        'sweeps %s' % (what, res, yard[0], orth, yard[1], envelope(n, sweeps or 0),
                       'n/a' if ev is None else '%.3g' % ev, yard[2], sweeps))
  assert res <= FACTOR * yard[0], '%s: residual %.4g u against %d x %.4g u' % (what, res, FACTOR, yard[0])
  assert orth <= FACTOR * yard[1], '%s: orthogonality %.4g u against %d x %.4g u' % (what, orth, FACTOR, yard[1])
  if ev is not None:
    assert ev <= FACTOR * yard[2], '%s: eigenvalues %.4g u against %d x %.4g u' % (what, ev, FACTOR, yard[2])
  if sweeps is None:
    pass
  elif sweeps == 0:
    assert orth == 0, '%s: no sweep, yet orth = %.4g u' % (what, orth)
  else:
    assert orth <= envelope(n, sweeps), '%s: orth %.4g u above the envelope %.4g u' % (what, orth,
                                                                                       envelope(n, sweeps))
  return res, orth, ev


def check_form(w, V):
  """Ascending eigenvalues; every column's first entry of largest magnitude is
  positive."""
  assert np.all(w[1:] >= w[:-1]), 'the eigenvalues are not ascending'
  for j in range(V.shape[1]):
    i = int(np.argmax(np.abs(V[:, j])))
    assert V[i, j] > 0, 'column %d: the entry of largest magnitude is not positive' % j


# -------------------------------------------------------------- test double
class EighFakeBackend(LinalgFakeBackend):
  """LinalgFakeBackend + ``syevj`` by scipy, with the kernel's ordering, sign
  rule and ``info`` convention (1 sweep reported for a converged matrix, 0 for
  the zero matrix and n == 1)."""

  def syevj(self, A, uplo='L'):
    a = _np(A)
    assert uplo in ('L', 'U') and a.ndim in (2, 3) and a.shape[-1] == a.shape[-2]
    assert a.dtype in (np.float32, np.float64)
    n = a.shape[-1]
    stack = a.reshape((-1, n, n))
    W = np.empty((stack.shape[0], n), a.dtype)
    V = np.empty(stack.shape, a.dtype)
    info = np.zeros(stack.shape[0], np.int32)
    for b, mat in enumerate(stack):
      tri = np.tril(mat) if uplo == 'L' else np.triu(mat)
      strict = np.tril(mat, -1) if uplo == 'L' else np.triu(mat, 1)
      with np.errstate(all='ignore'):
        full = tri + strict.T
      if not np.all(np.isfinite(full)):
        W[b], V[b], info[b] = np.nan, np.nan, -1
      elif not np.any(full) or n == 1:
        W[b], V[b], info[b] = np.diag(full), np.eye(n, dtype=a.dtype), 0
      else:
        W[b], V[b] = canonical(*lapack_eigh(np.ascontiguousarray(full)))
        info[b] = 1
    self.calls.append('syevj')
    return (torch.as_tensor(W.reshape(a.shape[:-1])), torch.as_tensor(V.reshape(a.shape)),
            torch.as_tensor(info))


# -------------------------------------------------------------- the drivers
def low_rank(m, n, k, seed):
  """U diag(linspace(6, 3, k + 1)) V^T of exact rank k + 1: the Krylov space of
  the (k + 2)-step Lanczos iteration is exhausted exactly at its last step."""
  r = np.random.RandomState(seed)
  U, _ = np.linalg.qr(r.standard_normal((m, k + 1)))
  V, _ = np.linalg.qr(r.standard_normal((n, k + 1)))
  return (U * np.linspace(6, 3, k + 1)).dot(V.T)


def check_drivers(W):
  """The reference's test_svds restated on a dense float64 matrix, and
  lanczos.solve on its Gram matrix, over row tiles for ``W`` workers."""
  from spartan_amd import expr
  from spartan_amd.examples.lanczos import solve
  from spartan_amd.examples.svd import svds
  for (m, n), k in (((80, 30), 6), ((60, 24), 10)):
    dense = low_rank(m, n, k, k)
    A = expr.from_numpy(dense, tile_hint=(-(-m // W), n))
    U, S, VT = svds(A, k)
    assert isinstance(U, np.ndarray) and isinstance(S, np.ndarray) and isinstance(VT, np.ndarray)
    assert U.shape == (m, k) and S.shape == (k,) and VT.shape == (k, n)
    U2, S2, VT2 = np.linalg.svd(dense, full_matrices=False)
    assert np.allclose(np.absolute(U), np.absolute(U2[:, :k]))
    assert np.allclose(np.absolute(S), np.absolute(S2[:k]))
    assert np.allclose(np.absolute(VT), np.absolute(VT2[:k]))
    G = dense.T.dot(dense)
    Ge = expr.from_numpy(G, tile_hint=(-(-n // W), n))
    d, s = solve(Ge, Ge, k, True)
    assert d.shape == (k,) and s.shape == (n, k)
    assert np.allclose(d, S2[:k] ** 2)
    assert np.allclose(np.absolute(s), np.absolute(VT2[:k].T))
