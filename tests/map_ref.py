"""Host-only reference for the generated map kernels (codegen.Emitter.op_expr):
which ufuncs are lowered for which dtypes, fixed operand vectors that hold the
values where lowerings go wrong, and NumPy's own result for them.  No GPU, no
torch.

Two classes of op:

* exact   -- the kernel must reproduce NumPy's result in the resolved dtype bit
             for bit (NaN payloads free): ``expected_exact`` is the ufunc itself.
* rounded -- math-library functions: ``expected_rounded`` is the same ufunc in
             np.longdouble (64-bit mantissa; mpmath at 120 bits where the
             platform's long double is narrower), compared through ``ulps``.

Inputs left out, at the generator, because NumPy's own result is
platform-defined or an exception (nothing is dropped at run time):

* float -> integer casts of NaN, +-inf or values outside the target's range;
* integer (and bool) ``reciprocal`` of 0;
* integer ``power`` with a negative exponent.

Integer division and remainder by 0, ``min // -1`` and wrapped integer
``power`` overflow all stay.
"""
import functools

import numpy as np

F32, F64 = np.dtype(np.float32), np.dtype(np.float64)
I8, U8, I16, I32, I64 = (np.dtype(t) for t in (np.int8, np.uint8, np.int16, np.int32, np.int64))
B = np.dtype(np.bool_)

FLOATS = (F32, F64)
INTS = (I8, U8, I16, I32, I64)
SUPPORTED = FLOATS + INTS + (B,)  # what codegen.CTYPE lowers
# everything a (op, dtype) lowering is attempted for on the CPU: SUPPORTED plus
# the dtypes the codegen documents it refuses
CANDIDATES = SUPPORTED + tuple(np.dtype(t) for t in (np.float16, np.uint16, np.uint32, np.uint64))

_ALL, _NUM = SUPPORTED, FLOATS + INTS
_WIDE = FLOATS + (I16, I32, I64)  # float functions: int8 / uint8 / bool inputs resolve to float16, not lowered


def _t(arity, cls, dtypes):
  return {'arity': arity, 'cls': cls, 'dtypes': tuple(dtypes)}


# name -> arity, class and the input dtypes it lowers for (both operands of a
# binary op have that dtype).  test_map_ref.py asserts that this table lists
# every name op_expr lowers and that exactly these (op, dtype) pairs lower,
# the rest of CANDIDATES raising the codegen's TypeError / NotImplementedError.
OPS = {
    'add': _t(2, 'exact', _ALL), 'subtract': _t(2, 'exact', _NUM), 'multiply': _t(2, 'exact', _ALL),
    'true_divide': _t(2, 'exact', _ALL), 'divide': _t(2, 'exact', _ALL),
    'floor_divide': _t(2, 'exact', _ALL), 'remainder': _t(2, 'exact', _ALL), 'mod': _t(2, 'exact', _ALL),
    'negative': _t(1, 'exact', _NUM), 'positive': _t(1, 'exact', _NUM), 'absolute': _t(1, 'exact', _ALL),
    'square': _t(1, 'exact', _ALL), 'reciprocal': _t(1, 'exact', _ALL), 'sign': _t(1, 'exact', _NUM),
    'maximum': _t(2, 'exact', _ALL), 'minimum': _t(2, 'exact', _ALL),
    'fmax': _t(2, 'exact', _ALL), 'fmin': _t(2, 'exact', _ALL),
    'equal': _t(2, 'exact', _ALL), 'not_equal': _t(2, 'exact', _ALL), 'less': _t(2, 'exact', _ALL),
    'less_equal': _t(2, 'exact', _ALL), 'greater': _t(2, 'exact', _ALL), 'greater_equal': _t(2, 'exact', _ALL),
    'logical_and': _t(2, 'exact', _ALL), 'logical_or': _t(2, 'exact', _ALL), 'logical_xor': _t(2, 'exact', _ALL),
    'logical_not': _t(1, 'exact', _ALL),
    'isnan': _t(1, 'exact', _ALL), 'isinf': _t(1, 'exact', _ALL), 'isfinite': _t(1, 'exact', _ALL),
    'floor': _t(1, 'exact', FLOATS), 'ceil': _t(1, 'exact', FLOATS), 'trunc': _t(1, 'exact', FLOATS),
    'rint': _t(1, 'exact', _WIDE), 'fabs': _t(1, 'exact', _WIDE), 'sqrt': _t(1, 'exact', _WIDE),
    'fmod': _t(2, 'exact', FLOATS),
    'power': _t(2, 'mixed', _ALL),  # integer power is exact, float power rounded: see op_class
    'arctan2': _t(2, 'rounded', _WIDE), 'hypot': _t(2, 'rounded', _WIDE),
}
for _n in ('exp', 'log', 'sin', 'cos', 'tan', 'tanh', 'sinh', 'cosh', 'arcsin', 'arccos', 'arctan', 'exp2', 'log2',
           'log10', 'expm1', 'log1p', 'cbrt'):
  OPS[_n] = _t(1, 'rounded', _WIDE)


def resolve(op, dtype, scalar=None):
  """(input dtypes, result dtype) of ``op`` on ``dtype`` arrays (second operand
  a Python scalar of type ``scalar`` if given), by NumPy's own resolution."""
  uf = getattr(np, op)
  keys = (np.dtype(dtype),) * uf.nin
  if scalar is not None:
    keys = (keys[0], scalar)
  res = uf.resolve_dtypes(keys + (None,))
  return tuple(np.dtype(d) for d in res[:uf.nin]), np.dtype(res[uf.nin])


def op_class(op, dtype):
  """'exact' or 'rounded' for ``op`` on ``dtype`` inputs."""
  c = OPS[op]['cls']
  if c != 'mixed':
    return c
  return 'rounded' if resolve(op, dtype)[0][0].kind == 'f' else 'exact'


def pairs():
  """Every (op, dtype) the GPU value tests run, in a fixed order."""
  return [(op, dt) for op in sorted(OPS) for dt in OPS[op]['dtypes']]


# ------------------------------------------------------------------ specials
def float_specials(dtype):
  fi = np.finfo(dtype)
  v = [0.0, 1.0, 0.5, 1.5, 2.5, np.inf, fi.max, fi.tiny, fi.smallest_subnormal, 1e-3, 1e3, np.pi / 2]
  out = []
  for x in v:
    out += [x, -x]
  return np.array(out + [np.nan], dtype=dtype)


def int_specials(dtype):
  ii = np.iinfo(dtype)
  v = [0, 1, -1, 2, -2, 3, -3, 7, -7, ii.min, ii.min + 1, ii.max - 1, ii.max]
  if np.dtype(dtype).itemsize == 8:
    v += [2 ** 53 + 1, -(2 ** 53 + 1)]
  v = sorted(set(x for x in v if ii.min <= x <= ii.max))
  return np.array(v, dtype=dtype)


def specials(dtype):
  dtype = np.dtype(dtype)
  if dtype.kind == 'f':
    return float_specials(dtype)
  if dtype.kind == 'b':
    return np.array([False, True])
  return int_specials(dtype)


def scalars(op, dtype):
  """Three Python scalars from the specials for the Sc operand of a binary op."""
  dtype = np.dtype(dtype)
  if dtype.kind == 'f':
    return [-1.5, float('inf'), 1e-3]  # 1e-3: a double that must round to the array's fp32 first
  if dtype.kind == 'b':
    return [True, False, True]
  ii = np.iinfo(dtype)
  third = 2 ** 53 + 1 if dtype.itemsize == 8 else int(ii.max)  # int64: exact above 2^53
  second = 7 if (dtype.kind == 'u' or op == 'power') else -7
  return [3, second, third]


def decimal_grid(dtype):
  """a = k * 0.1 (k in -50..50) against b = m * 0.1 (m in -19..19, no 0), rounded
  to the dtype; for integer dtypes k against m themselves."""
  dtype = np.dtype(dtype)
  k, m = np.arange(-50, 51), np.array([x for x in range(-19, 20) if x != 0])
  kk, mm = (x.ravel() for x in np.meshgrid(k, m, indexing='ij'))
  if dtype.kind == 'f':
    return (kk * 0.1).astype(dtype), (mm * 0.1).astype(dtype)
  if dtype.kind == 'b':
    return (kk % 2 == 0), (mm % 3 == 0)
  if dtype.kind == 'u':
    kk, mm = np.abs(kk), np.abs(mm)
  return kk.astype(dtype), mm.astype(dtype)


def _rng(op, dtype, salt=0):
  return np.random.default_rng([sum(ord(c) for c in op), np.dtype(dtype).num, salt])


def _draws(op, dtype, n, salt=0):
  """n seeded general-purpose values: floats over many magnitudes and both
  signs, integers over the whole range with half of them small."""
  dtype = np.dtype(dtype)
  r = _rng(op, dtype, salt)
  if dtype.kind == 'f':
    v = r.standard_normal(n) * 10.0 ** r.integers(-3, 4, n)
    return v.astype(dtype)
  if dtype.kind == 'b':
    return r.integers(0, 2, n).astype(bool)
  ii = np.iinfo(dtype)
  wide = r.integers(ii.min, ii.max, n, dtype=dtype, endpoint=True)
  small = r.integers(max(ii.min, -20), min(ii.max, 20), n, endpoint=True).astype(dtype)
  return np.where(r.integers(0, 2, n) == 0, wide, small).astype(dtype)


def _around(x, dtype):
  """x rounded to dtype, with its two neighbours."""
  x = np.array(x, dtype=np.longdouble).astype(dtype)
  return [np.nextafter(x, dtype.type(-np.inf)), x, np.nextafter(x, dtype.type(np.inf))]


def _domain_unary(op, dtype):
  """Values inside the domain of a rounded unary op (finite, normal results) and
  its edges, for a float dtype."""
  fi = np.finfo(dtype)
  r = _rng(op, dtype, 1)
  n = 2000
  ld = np.longdouble
  big = 1e30 if dtype == F32 else 1e22
  tiny_args = [1e-10, -1e-10, 1e-20, -1e-20]
  # where exp-like functions overflow, lose normal results and underflow to zero
  emax, emin, esub = (float(np.log(ld(fi.max))), float(np.log(ld(fi.tiny))),
                      float(np.log(ld(fi.smallest_subnormal))))
  if op in ('exp', 'expm1'):
    dom = r.uniform(emin, emax, n)
    edge = [e for x in (emax, emin, esub, esub - np.log(2.0)) for e in _around(x, dtype)]
    edge += tiny_args if op == 'expm1' else []
  elif op == 'exp2':
    dom = r.uniform(fi.minexp, fi.maxexp, n)
    edge = [e for x in (fi.maxexp, fi.minexp, fi.minexp - fi.nmant, fi.minexp - fi.nmant - 1)
            for e in _around(x, dtype)]
  elif op in ('sinh', 'cosh'):
    dom = r.uniform(-emax, emax, n)
    edge = [e for x in (emax + np.log(2.0), -emax - np.log(2.0)) for e in _around(x, dtype)]
  elif op in ('log', 'log2', 'log10', 'sqrt', 'cbrt'):
    dom = np.exp(r.uniform(emin, emax, n))
    edge = [0.0, -0.0, -1.0, -fi.tiny]
  elif op == 'log1p':
    dom = np.concatenate([r.uniform(-0.99, 10.0, n // 2), np.exp(r.uniform(-40.0, 40.0, n // 2))])
    edge = [-1.0, np.nextafter(dtype.type(-1), dtype.type(-2)), -2.0] + tiny_args
  elif op in ('arcsin', 'arccos'):
    dom = r.uniform(-1.0, 1.0, n)
    one = dtype.type(1)
    edge = [1.0, -1.0, np.nextafter(one, dtype.type(2)), -np.nextafter(one, dtype.type(2))]
  elif op in ('sin', 'cos', 'tan'):
    dom = r.uniform(-100.0, 100.0, n)
    edge = [1e5, -1e5, big, -big]
  elif op == 'tanh':
    dom = r.uniform(-20.0, 20.0, n)
    edge = [1e3, -1e3] + tiny_args
  else:  # arctan and the exact float functions: any magnitude
    dom = r.standard_normal(n) * 10.0 ** r.integers(-3, 6, n)
    edge = [k + 0.5 for k in range(-6, 6)] + [2.0 ** fi.nmant + 1, -(2.0 ** fi.nmant) - 1, 2.0 ** (fi.nmant - 1) + 0.5]
  return np.concatenate([np.asarray(dom).astype(dtype), np.array(edge, dtype=dtype)])


def _domain_binary(op, dtype):
  """The named edge cases of the rounded binary ops and in-domain draws."""
  r = _rng(op, dtype, 2)
  n = 1000
  inf, nan = np.inf, np.nan
  if op == 'power':
    a = np.concatenate([r.uniform(0.1, 10.0, n), -r.integers(1, 8, 64).astype(float)])
    b = np.concatenate([r.uniform(-10.0, 10.0, n), r.integers(-6, 7, 64).astype(float)])
    ea = [0.0, -0.0, -2.0, -2.0, -2.0, -2.0, 2.0, 2.0, 0.5, 0.5, -0.5, -1.0, 1.0, 1.0]
    eb = [0.0, 0.0, 0.5, 3.0, 4.0, -3.0, inf, -inf, inf, -inf, inf, inf, inf, nan]
  elif op == 'arctan2':
    a, b = r.standard_normal(n), r.standard_normal(n)
    ea = [1.0, 1.0, -1.0, -1.0, 0.0, 0.0, -0.0, -0.0, 0.0, -0.0, 1.0, -1.0]
    eb = [1.0, -1.0, 1.0, -1.0, 0.0, -0.0, 0.0, -0.0, -1.0, -1.0, 0.0, -0.0]
  else:  # hypot
    a, b = (r.standard_normal(n) * 10.0 ** r.integers(-3, 4, n) for _ in range(2))
    ea, eb = [inf, nan, -inf, 3.0], [nan, inf, nan, 4.0]
  return (np.concatenate([a, ea]).astype(dtype), np.concatenate([b, eb]).astype(dtype))


@functools.lru_cache(maxsize=None)
def _inputs(op, dtype):
  dtype = np.dtype(dtype)
  sp = specials(dtype)
  if OPS[op]['arity'] == 1:
    v = [sp, _draws(op, dtype, 2000)]
    if dtype.kind == 'f':
      v.append(_domain_unary(op, dtype))
    x = np.concatenate(v).astype(dtype)
    if op == 'reciprocal' and dtype.kind != 'f':
      x = x[x != 0]  # integer reciprocal of 0: NumPy's value is platform-defined (left out, see module doc)
    args = (x,)
  else:
    ca, cb = (m.ravel() for m in np.meshgrid(sp, sp, indexing='ij'))  # the full cross product
    ga, gb = decimal_grid(dtype)
    va, vb = [ca, ga, _draws(op, dtype, 2000, 3)], [cb, gb, _draws(op, dtype, 2000, 4)]
    if dtype.kind == 'f':  # zero remainders of both signs against divisors of both signs
      va.append(np.array([4.0, -4.0, 4.0, -4.0, 6.0, -6.0]))
      vb.append(np.array([-2.0, 2.0, 2.0, -2.0, -1.5, 1.5]))
    if dtype.kind == 'f' and op in ('power', 'arctan2', 'hypot'):
      da, db = _domain_binary(op, dtype)
      va.append(da)
      vb.append(db)
    a, b = np.concatenate(va).astype(dtype), np.concatenate(vb).astype(dtype)
    if op == 'power' and dtype.kind == 'i':
      keep = b >= 0  # integer power with a negative exponent raises in NumPy (left out, see module doc)
      a, b = a[keep], b[keep]
    args = (a, b)
  for x in args:
    x.setflags(write=False)
  return args


def inputs(op, dtype):
  """The fixed operand vectors of (op, dtype): a tuple of ``arity`` read-only
  1-d arrays of ``dtype`` and equal length."""
  return _inputs(op, np.dtype(dtype))


def cast_inputs(src, dst):
  """Source values for Cast(src -> dst): specials and draws, without the float
  -> integer conversions C and NumPy leave platform-defined (NaN, +-inf, out of
  the target's range)."""
  src, dst = np.dtype(src), np.dtype(dst)
  x = np.concatenate([specials(src), _draws('cast', src, 2000)]).astype(src)
  if src.kind == 'f' and dst.kind in 'iu':
    ii = np.iinfo(dst)
    with np.errstate(all='ignore'):
      t = np.trunc(x.astype(np.longdouble))
    x = x[np.isfinite(x) & (t >= ii.min) & (t <= ii.max)]
  return x


# ---------------------------------------------------------------- references
def expected_exact(op, args):
  """NumPy's ufunc on ``args`` (arrays in their dtypes; a Python scalar stays a
  weak scalar) -- the value the kernel must reproduce bit for bit."""
  with np.errstate(all='ignore'):
    return np.asarray(getattr(np, op)(*args))


def bits(a):
  """A view that compares as the issue's exact rule: integers for the floats'
  bit patterns with every NaN mapped to one pattern (payload free), so signed
  zeros differ and all else compares by value."""
  a = np.ascontiguousarray(a)
  if a.dtype.kind != 'f':
    return a
  u = a.view(np.uint32 if a.dtype == F32 else np.uint64).copy()
  u[np.isnan(a)] = np.array(np.nan, dtype=a.dtype).view(u.dtype)
  return u


def have_longdouble():
  return np.finfo(np.longdouble).nmant >= 63


def have_reference():
  if have_longdouble():
    return True
  try:
    import mpmath  # noqa: F401
    return True
  except ImportError:
    return False


_MP = {'arcsin': 'asin', 'arccos': 'acos', 'arctan': 'atan', 'arctan2': 'atan2', 'power': 'power'}


def expected_rounded(op, args):
  """``op`` on ``args`` (arrays already in the resolved float dtype) evaluated
  in np.longdouble; with a narrower long double, by mpmath at 120 bits
  (returned as longdouble all the same)."""
  if have_longdouble():
    with np.errstate(all='ignore'):
      return np.asarray(getattr(np, op)(*[np.asarray(a).astype(np.longdouble) for a in args]))
  import mpmath  # pragma: no cover - only where long double is a double
  mpmath.mp.prec = 120
  f = {'exp2': lambda x: mpmath.power(2, x), 'log2': lambda x: mpmath.log(x, 2), 'log1p': mpmath.log1p,
       'expm1': mpmath.expm1, 'cbrt': mpmath.cbrt}.get(op) or getattr(mpmath, _MP.get(op, op))
  out = np.empty(len(args[0]), dtype=np.longdouble)
  with np.errstate(all='ignore'):
    plain = np.asarray(getattr(np, op)(*[np.asarray(a, dtype=np.float64) for a in args]))
  for i in range(len(out)):
    xs = [float(a[i]) for a in args]
    if not all(np.isfinite(xs)) or not np.isfinite(plain[i]) or plain[i] == 0:
      out[i] = plain[i]  # special values: the class and sign are what is compared
    else:
      out[i] = np.longdouble(float(f(*[mpmath.mpf(x) for x in xs])))
  return out


def ulps(got, want_ld, dtype):
  """|got - want| in units of the dtype's spacing at ``want`` (the subnormal
  spacing below the smallest normal).  Values past the largest finite are
  taken as 2^(emax+1) on both sides, so an overflow to inf counts like any
  other rounding.  Meaningful where ``want`` is finite and not zero; a NaN
  ``got`` there counts as infinitely wrong."""
  fi = np.finfo(dtype)
  ld = np.longdouble
  top = np.ldexp(ld(1), fi.maxexp)
  with np.errstate(all='ignore'):
    g = np.clip(np.asarray(got).astype(ld), -top, top)
    w = np.clip(np.asarray(want_ld, dtype=ld), -top, top)
    _, ex = np.frexp(np.abs(w))
    ex = np.clip(ex - 1, fi.minexp, fi.maxexp - 1)
    err = np.abs(g - w) / np.ldexp(ld(1), ex - fi.nmant)
  return np.where(np.isnan(g), np.inf, err)


def numeric_mask(want_ld):
  """Where a rounded result is compared by value (finite and not zero); the
  rest (NaN, +-inf, +-0) is compared by class and sign."""
  w = np.asarray(want_ld)
  return np.isfinite(w) & (w != 0)


def same_class(got, want_ld):
  """Per element: ``got`` has the class and sign of a NaN / +-inf / +-0 ``want``."""
  g, w = np.asarray(got), np.asarray(want_ld)
  with np.errstate(all='ignore'):
    return np.where(np.isnan(w), np.isnan(g),
                    np.where(np.isinf(w), np.isinf(g) & (np.signbit(g) == np.signbit(w)),
                             (g == 0) & (np.signbit(g) == np.signbit(w))))
