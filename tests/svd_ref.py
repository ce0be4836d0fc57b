"""Shared by tests/test_svd.py and tests/test_svd_gpu.py: the data kinds, the
error ratios, the yardstick and the CPU test double of DESIGN.md 3.25.

With u the unit roundoff of the data's dtype, evaluated in np.longdouble:

  res   = ||A - U diag(s) Vt||_F / (u ||A||_F)   (exactly 0 for the zero matrix),
  orthV = ||Vt Vt^T - I||_2 / u,
  orthU = ||U1^T U1 - I||_2 / u over the columns U1 of U with s_j > 0; the
          columns with s_j == 0 must be exactly zero (the contract),
  sv    = max_j |s_j - sigma_j| / (u sigma_max)   where the spectrum is prescribed,
  rel   = max_j |s_j - sigma_j| / (u sigma_j)     for the kind 'graded' only, with
          sigma from ``jacobi_svd_model`` run one precision up on the same
          rounded data (float64 for float32 data; np.longdouble for float64 data
          where it is wider, else ``rel`` is skipped).  This ratio is the reason
          to use a one-sided Jacobi method: it stays a modest multiple of u over
          a grading of 1e6 / 1e15, which a norm-wise bound (u sigma_max, all
          that LAPACK's gesvd promises) does not give.

The yardstick, per (dtype, m, n), is the largest ratio over all data kinds of

  * ``jacobi_svd_model``: a NumPy restatement, in the data's own dtype, of the
    method spx_gesvj is specified to run.  It is written from the
    specification, not from the kernel, and shares no code with it;
  * LAPACK: ``scipy.linalg.svd(lapack_driver='gesvd')`` in the data's dtype;

for ``rel`` it is the model's ratio alone.  A result passes within FACTOR = 4 x
the yardstick: the margin of qr_ref / eigh_ref, for a different but equally
valid order of sums.

So that the yardstick cannot hide a broken model, eigh_ref's unconditional
envelope holds for orthV besides: at most 4 n sqrt(S) u for S sweeps, and
exactly 0 for S == 0.
"""
import numpy as np
import torch

from fake_backend import _np
from eigh_ref import EighFakeBackend, envelope, low_rank, round_robin  # noqa: F401  (re-exported)
from linalg_ref import LD, _wide, same_bits, unit_roundoff  # noqa: F401  (re-exported)
from qr_ref import QrFakeBackend

KINDS = ('gauss', 'illcond', 'rankdef', 'cluster', 'graded', 'diag', 'dup', 'ones', 'zero')
FACTOR = 4
SWEEP_MAX = 64


# ------------------------------------------------------------------- data
def _with_spectrum(sig, m, n, r):
  """U diag(sig) V^T in np.longdouble, U (m, n) and V (n, n) the products of n
  random Householder reflectors each."""
  M = np.zeros((m, n), LD)
  M[np.arange(n), np.arange(n)] = sig.astype(LD)
  for _ in range(n):
    v = r.standard_normal(m).astype(LD)
    v /= np.sqrt((v * v).sum())
    M = M - 2 * np.outer(v, v.dot(M))
    w = r.standard_normal(n).astype(LD)
    w /= np.sqrt((w * w).sum())
    M = M - 2 * np.outer(M.dot(w), w)
  return M


def dup_columns(n):
  """(p, q, z) of the kind 'dup': columns p and q are equal and column z is
  zero.  (p, q) is a pair of the tournament's first round, so the two columns
  meet before anything else has touched them."""
  if n < 2:
    return None
  if n == 2:
    return 0, 1, None
  p, q = round_robin(n + (n & 1))[0][1]
  return p, q, 0


def svd_data(kind, m, n, dtype, seed=0):
  """(A, sigma): an (m, n) matrix of ``dtype``, m >= n, and its prescribed
  singular values in descending order (np.longdouble), or None.  kind:
    'gauss'    standard normal;
    'illcond'  sigma = logspace(0, -5 | -13) (float32 | float64);
    'rankdef'  half the spectrum exactly 0 (before the rounding to dtype);
    'cluster'  two thirds of the spectrum exactly 1, the rest within 1e-3;
    'graded'   Gaussian times the column scaling logspace(0, -6 | -15);
    'diag'     small integers on the diagonal (exact in every dtype);
    'dup'      Gaussian with two equal columns and one zero column;
    'ones'     all ones;
    'zero'     all zeros."""
  dt = np.dtype(dtype)
  f32 = dt == np.float32
  r = np.random.RandomState(seed + 7919 * m + 104729 * n + (0 if f32 else 13))
  sig = None
  if kind == 'gauss':
    A = r.standard_normal((m, n))
  elif kind in ('illcond', 'rankdef', 'cluster'):
    if kind == 'illcond':
      sig = np.logspace(0, -5 if f32 else -13, n)
    elif kind == 'rankdef':
      sig = np.concatenate([1.0 + r.uniform(size=n - n // 2), np.zeros(n // 2)])
    else:
      k = (2 * n) // 3
      sig = np.concatenate([np.ones(k), 1.0 + 1e-3 * r.uniform(-1, 1, size=n - k)])
    sig = np.sort(sig.astype(LD))[::-1]
    A = _with_spectrum(sig, m, n, r)
  elif kind == 'graded':
    A = r.standard_normal((m, n)) * np.logspace(0, -6 if f32 else -15, n)[None, :]
  elif kind == 'diag':
    d = ((np.arange(n) * 5) % 11 - 4).astype(np.float64)
    A = np.zeros((m, n))
    A[np.arange(n), np.arange(n)] = d
    sig = np.sort(np.abs(d).astype(LD))[::-1]
  elif kind == 'dup':
    A = r.standard_normal((m, n))
    cols = dup_columns(n)
    if cols:
      p, q, z = cols
      A[:, q] = A[:, p]
      if z is not None:
        A[:, z] = 0.0
  elif kind == 'ones':
    A = np.ones((m, n))
    sig = np.concatenate([[np.sqrt(LD(m * n))], np.zeros(n - 1, LD)])
  elif kind == 'zero':
    A = np.zeros((m, n))
    sig = np.zeros(n, LD)
  else:
    raise ValueError(kind)
  return np.ascontiguousarray(np.asarray(A).astype(dt)), sig  # rounded once


# ----------------------------------------------------------------- ratios
def _norm2(e, u):
  scale = np.abs(e).max() if e.size else 0
  if not scale > 0:
    return 0.0
  # the 2-norm of the scaled matrix in double: 1e-16 relative, on a quantity of a few u
  return float(LD(np.linalg.norm((e / scale).astype(np.float64), 2)) * scale / u)


def svd_ratios(A, U, s, Vt, sigma=None):
  """(res, orthV, orthU, sv) in units of u; sv is None without a prescribed
  spectrum.  Asserts the zero-column contract."""
  dt = A.dtype
  _wide(dt)
  m, n = A.shape
  assert U.shape == (m, n) and s.shape == (n,) and Vt.shape == (n, n)
  assert U.dtype == dt and s.dtype == dt and Vt.dtype == dt
  assert np.all(np.isfinite(U)) and np.all(np.isfinite(s)) and np.all(np.isfinite(Vt)), 'non-finite entries'
  u = unit_roundoff(dt)
  a, ul, sl, vl = A.astype(LD), U.astype(LD), s.astype(LD), Vt.astype(LD)
  d = a - (ul * sl[None, :]).dot(vl)
  an = np.sqrt((a * a).sum())
  if an == 0:
    assert not np.any(d != 0), 'a nonzero residual for the zero matrix'
    res = 0.0
  else:
    res = float(np.sqrt((d * d).sum()) / (u * an))
  orthV = _norm2(vl.dot(vl.T) - np.eye(n, dtype=LD), u)
  live = s > 0
  assert not np.any(U[:, ~live]), 'a nonzero column of U for an exactly zero singular value'
  u1 = ul[:, live]
  orthU = _norm2(u1.T.dot(u1) - np.eye(u1.shape[1], dtype=LD), u)
  sv = None
  if sigma is not None:
    top = sigma.max() if n else 0
    diff = np.abs(sl - sigma.astype(LD))
    if top == 0:
      assert not np.any(diff != 0), 'a nonzero singular value for the zero spectrum'
      sv = 0.0
    else:
      sv = float(diff.max() / (u * top))
  return res, orthV, orthU, sv


def rel_ratio(s, sigma, dtype):
  """max_j |s_j - sigma_j| / (u sigma_j) over the sigma_j > 0."""
  u = unit_roundoff(dtype)
  sl, sg = s.astype(LD), sigma.astype(LD)
  pos = sg > 0
  assert not np.any(sl[~pos] != 0)
  return float(np.max(np.abs(sl[pos] - sg[pos]) / (u * sg[pos]))) if np.any(pos) else 0.0


def canonical(U, s, Vt):
  """(U, s, Vt) in the contract's form: descending, ties by index; every row
  of Vt with its entry of largest magnitude (the first on a tie) positive, the
  column of U carrying the sign; an exactly zero s_j with a zero column of U."""
  order = np.argsort(-s, kind='stable')
  U, s, Vt = U[:, order].copy(), s[order].copy(), Vt[order].copy()
  for j in range(Vt.shape[0]):
    i = int(np.argmax(np.abs(Vt[j])))  # the first maximum
    if Vt[j, i] < 0:
      Vt[j] = -Vt[j]
      U[:, j] = -U[:, j]
    if s[j] == 0:
      U[:, j] = 0
  return np.ascontiguousarray(U), np.ascontiguousarray(s), np.ascontiguousarray(Vt)


def check_form(s, Vt):
  """Descending non-negative singular values; every row of Vt has its first
  entry of largest magnitude positive."""
  assert np.all(s >= 0) and np.all(s[:-1] >= s[1:]), 'the singular values are not descending and non-negative'
  for j in range(Vt.shape[0]):
    i = int(np.argmax(np.abs(Vt[j])))
    assert Vt[j, i] > 0, 'row %d of Vt: the entry of largest magnitude is not positive' % j


# --------------------------------------------------------------- the model
def jacobi_svd_model(A, sweep_max=SWEEP_MAX):
  """(U, s, Vt, sweeps) of ``A`` (m >= n) by the specified method, every
  operation in A's dtype (the final norms in a wider type); sweeps == -1 (and
  NaN results) where it does not converge or A is not finite."""
  dt = A.dtype
  T = dt.type
  m, n = A.shape
  wide = np.float64 if dt == np.float32 else LD
  nan = (np.full((m, n), np.nan, dt), np.full(n, np.nan, dt), np.full((n, n), np.nan, dt), -1)
  if n == 0:
    return np.zeros((m, 0), dt), np.zeros(0, dt), np.zeros((0, 0), dt), 0
  big = np.abs(A).max()
  if not np.isfinite(big):
    return nan
  if big == 0:
    return np.zeros((m, n), dt), np.zeros(n, dt), np.eye(n, dtype=dt), 0
  e = int(np.floor(np.log2(float(big))))
  while T(2) ** e > big:
    e -= 1
  while T(2) ** (e + 1) <= big:
    e += 1
  g = np.ldexp(A, -e).astype(dt)
  V = np.eye(n, dtype=dt)
  u = np.finfo(dt).eps / 2
  tol = T(np.sqrt(T(m)) * u)
  tiny = T(np.finfo(dt).tiny / u)  # a column whose squared norm is at most this counts as a zero column
  one = T(1)
  sweeps = 0
  if n > 1:
    mm = n + (n & 1)
    rounds = [(np.array([p for p, q in pairs if q < n]), np.array([q for p, q in pairs if q < n]))
              for pairs in round_robin(mm)]
    sweeps = -1
    with np.errstate(all='ignore'):
      for sweep in range(sweep_max):
        rotated = False
        for P, Q in rounds:
          gp, gq = g[:, P], g[:, Q]
          app = (gp * gp).sum(0, dtype=dt)
          aqq = (gq * gq).sum(0, dtype=dt)
          apq = (gp * gq).sum(0, dtype=dt)
          hit = (app > tiny) & (aqq > tiny) & (np.abs(apq) > tol * np.sqrt(app) * np.sqrt(aqq))
          if not hit.any():
            continue
          rotated = True
          P, Q, app, aqq, apq = P[hit], Q[hit], app[hit], aqq[hit], apq[hit]
          theta = (aqq - app) / (T(2) * apq)
          at = np.abs(theta)
          # (from 1 / u on the formula rounds to 1 / (2 |theta|): written out, so that theta^2 cannot overflow)
          t = np.where(at >= T(1 / u), one / (T(2) * at), one / (at + np.sqrt(at * at + one))).astype(dt)
          t = np.where(theta < 0, -t, t).astype(dt)
          c = (one / np.sqrt(t * t + one)).astype(dt)
          s = (t * c).astype(dt)
          for M in (g, V):
            xp, xq = M[:, P], M[:, Q]
            M[:, P] = c * xp - s * xq
            M[:, Q] = s * xp + c * xq
        if not rotated:
          sweeps = sweep + 1
          break
    if sweeps < 0:
      return nan
  gw = g.astype(wide)
  ss = (gw * gw).sum(0)
  sc = np.where(ss > tiny, np.sqrt(ss), 0).astype(dt)  # the scaled singular values
  U = np.zeros((m, n), dt)
  live = sc > 0
  U[:, live] = g[:, live] / sc[live]
  U, s, Vt = canonical(U, np.ldexp(sc, e).astype(dt), V.T)
  return U, s, Vt, sweeps


def lapack_svd(A):
  from scipy.linalg import svd
  m, n = A.shape
  if n == 0:
    return np.zeros((m, 0), A.dtype), np.zeros(0, A.dtype), np.zeros((0, 0), A.dtype)
  U, s, Vt = svd(A, full_matrices=False, lapack_driver='gesvd', check_finite=False)
  assert U.dtype == A.dtype and s.dtype == A.dtype and Vt.dtype == A.dtype  # the data's own precision
  return U, s, Vt


# ------------------------------------------------------------ the yardstick
_YARD = {}
_MODEL = {}
_REL = {}


def model_run(kind, m, n, dtype, seed=0):
  """((res, orthV, orthU, sv), sweeps, s) of the model on one data kind (cached)."""
  key = (kind, m, n, np.dtype(dtype).str, seed)
  if key not in _MODEL:
    A, sig = svd_data(kind, m, n, dtype, seed)
    U, s, Vt, sweeps = jacobi_svd_model(A)
    assert sweeps >= 0, 'the model did not converge on %s' % (key,)
    _MODEL[key] = (svd_ratios(A, U, s, Vt, sig), sweeps, s)
  return _MODEL[key]


def yardstick(dtype, m, n, seed=0):
  """(Y_res, Y_orthV, Y_orthU, Y_sv): the largest ratios of the model and of
  LAPACK over KINDS at (dtype, m, n)."""
  key = (np.dtype(dtype).str, m, n, seed)
  if key not in _YARD:
    y = [0.0] * 4
    for kind in KINDS:
      A, sig = svd_data(kind, m, n, dtype, seed)
      for ratios in (model_run(kind, m, n, dtype, seed)[0], svd_ratios(A, *canonical(*lapack_svd(A)), sigma=sig)):
        for i, x in enumerate(ratios):
          if x is not None:
            y[i] = max(y[i], x)
    _YARD[key] = tuple(y)
  return _YARD[key]


TALL_KINDS = ('gauss', 'illcond', 'rankdef')


def tall_yardstick(dtype, m, n, seed=0):
  """The yardstick of the tall route (a TSQR, then the SVD of the n x n factor R
  by the same Jacobi method, then U = Q U_R): the larger of LAPACK's ratios over
  TALL_KINDS on the (m, n) data itself and of the direct route's yardstick at
  (n, n), which is what the SVD of R is held to (a Jacobi method is less
  orthogonal than a Householder-based one, so LAPACK alone is the wrong
  yardstick, as in eigh_ref) -- no model of the QR is needed --, with qr_ref's
  measured yardstick for Q added to ``res`` and ``orthU``, which inherit Q's
  errors: the SUM of the two yardsticks."""
  import qr_ref
  key = ('tall', np.dtype(dtype).str, m, n, seed)
  if key not in _YARD:
    y = [0.0] * 4
    for kind in TALL_KINDS:
      A, sig = svd_data(kind, m, n, dtype, seed)
      for i, x in enumerate(svd_ratios(A, *canonical(*lapack_svd(A)), sigma=sig)):
        if x is not None:
          y[i] = max(y[i], x)
    y = [max(a, b) for a, b in zip(y, yardstick(dtype, n, n, seed))]
    qres, qorth = qr_ref.yardstick(dtype, n, (m,), seed)
    _YARD[key] = (y[0] + qres, y[1], y[2] + qorth, y[3])
  return _YARD[key]


def rel_reference(m, n, dtype, seed=0):
  """(sigma, Y_rel) of the kind 'graded' at (m, n): the singular values of the
  model run one precision up on the same rounded data, and the model's own
  ``rel`` ratio against them; None where np.longdouble is not wider than the
  float64 data."""
  dt = np.dtype(dtype)
  key = (dt.str, m, n, seed)
  if key not in _REL:
    up = np.dtype(np.float64) if dt == np.float32 else np.dtype(LD)
    if np.finfo(up).nmant <= np.finfo(dt).nmant + 8:
      _REL[key] = None  # np.longdouble is double here: nothing to compare float64 against
    else:
      A, _ = svd_data('graded', m, n, dt, seed)
      _, sigma, _, sweeps = jacobi_svd_model(A.astype(up))
      assert sweeps >= 0
      _REL[key] = (sigma.astype(LD), rel_ratio(model_run('graded', m, n, dt, seed)[2], sigma, dt))
  return _REL[key]


def assert_ratios(A, U, s, Vt, sigma, sweeps, yard, what):
  """The ratios within FACTOR x the yardstick, and the envelope on orthV for
  the ``sweeps`` the solver reported (None: not known, no envelope); returns
  the ratios."""
  n = A.shape[1]
  res, orthV, orthU, sv = svd_ratios(A, U, s, Vt, sigma)
  print('%s: res %.3g u (yardstick %.3g), orthV %.3g u (yardstick %.3g, envelope %.3g), orthU %.3g u (yardstick '
        '%.3g), sv %s u (yardstick %.3g), sweeps %s'
        % (what, res, yard[0], orthV, yard[1], envelope(n, sweeps or 0), orthU, yard[2],
           'n/a' if sv is None else '%.3g' % sv, yard[3], sweeps))
  assert res <= FACTOR * yard[0], '%s: residual %.4g u against %d x %.4g u' % (what, res, FACTOR, yard[0])
  assert orthV <= FACTOR * yard[1], '%s: orthV %.4g u against %d x %.4g u' % (what, orthV, FACTOR, yard[1])
  assert orthU <= FACTOR * yard[2], '%s: orthU %.4g u against %d x %.4g u' % (what, orthU, FACTOR, yard[2])
  if sv is not None:
    assert sv <= FACTOR * yard[3], '%s: singular values %.4g u against %d x %.4g u' % (what, sv, FACTOR, yard[3])
  if sweeps is None:
    pass
  elif sweeps == 0:
    assert orthV == 0, '%s: no sweep, yet orthV = %.4g u' % (what, orthV)
  else:
    assert orthV <= envelope(n, sweeps), '%s: orthV %.4g u above the envelope %.4g u' % (what, orthV,
                                                                                         envelope(n, sweeps))
  return res, orthV, orthU, sv


def assert_rel(s, m, n, dtype, what, seed=0):
  """``rel`` of the 'graded' result ``s`` within FACTOR x the model's; says so
  where there is nothing wider to compare float64 with."""
  ref = rel_reference(m, n, dtype, seed)
  if ref is None:
    print('%s: rel skipped, np.longdouble is not wider than float64 here' % what)
    return None
  sigma, yard = ref
  rel = rel_ratio(s, sigma, dtype)
  print('%s: rel %.3g u (the model: %.3g)' % (what, rel, yard))
  # (rounding sigma to the dtype alone moves this ratio by up to 1 u)
  assert rel <= FACTOR * max(yard, 1.0), '%s: rel %.4g u against %d x %.4g u' % (what, rel, FACTOR, yard)
  return rel


# -------------------------------------------------------------- test double
class SvdFakeBackend(EighFakeBackend):
  """EighFakeBackend + qr_ref's ``geqr`` / ``orgqr`` (the tall route) +
  ``gesvj`` by scipy with the kernel's ordering, sign rule, zero-column rule and
  ``info`` convention (1 sweep reported for a converged matrix, 0 for the zero
  matrix and n == 1, -1 with NaN outputs for a matrix that is not finite)."""
  geqr = QrFakeBackend.geqr
  orgqr = QrFakeBackend.orgqr

  def gesvj(self, A, compute_uv=True):
    a = _np(A)
    assert a.ndim in (2, 3) and a.shape[-2] >= a.shape[-1] and a.dtype in (np.float32, np.float64)
    m, n = a.shape[-2:]
    stack = a.reshape((-1, m, n))
    nb = stack.shape[0]
    U, S, Vt = np.empty((nb, m, n), a.dtype), np.empty((nb, n), a.dtype), np.empty((nb, n, n), a.dtype)
    info = np.zeros(nb, np.int32)
    for b, mat in enumerate(stack):
      if not np.all(np.isfinite(mat)):
        U[b], S[b], Vt[b], info[b] = np.nan, np.nan, np.nan, -1
      elif not np.any(mat):
        U[b], S[b], Vt[b] = 0, 0, np.eye(n, dtype=a.dtype)
      else:
        U[b], S[b], Vt[b] = canonical(*lapack_svd(np.ascontiguousarray(mat)))
        info[b] = 0 if n == 1 else 1
    self.calls.append('gesvj')
    lead = a.shape[:-2]
    if not compute_uv:
      return None, torch.as_tensor(S.reshape(lead + (n,))), None, torch.as_tensor(info)
    return (torch.as_tensor(U.reshape(lead + (m, n))), torch.as_tensor(S.reshape(lead + (n,))),
            torch.as_tensor(Vt.reshape(lead + (n, n))), torch.as_tensor(info))
