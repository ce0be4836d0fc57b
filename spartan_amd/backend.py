"""Kernel backend: the device side of libspx.so + the generated-kernel JIT.

This is the only module that touches the GPU compute path: the JIT that
compiles generated kernels for gfx950, the reduce planner and ``HipBackend``,
which launches libspx.so's ahead-of-time kernels and the generated ones.  The
binding itself -- the ctypes signature table, ``load_library``, the dtype
codes and the plan / limit queries that need no GPU -- lives in ``binding``;
its public names are re-exported here, so ``backend.X`` keeps working.  Tests
may install a different backend object with ``set_backend`` to exercise the
host logic without a GPU; product code never does.

Tensors are PyTorch-ROCm device tensors (allocation and streams only); every
call passes raw pointers and the current HIP stream to the C ABI.
"""
import ctypes
import hashlib
import os
import subprocess
import tempfile
import threading
import weakref
from collections import namedtuple

import numpy as np

from . import binding, codegen
from .config import FLAGS
from .layout import broadcast_strides, coalesce, reduce_view, contiguous_strides
from .binding import (LIB_PATH, SPX_BOOL, SPX_I32, SPX_I64, SPX_F32, SPX_F64, OP_CODE, FILL_CONST, FILL_ARANGE,
                     FILL_UNIFORM, FILL_NORMAL, EXPORTED, SCAN_CHUNK, SORT_LDS_MAX, SORT_TILE, spx_dtype, torch_dtype,
                     np_dtype, load_library, mincost_tiling, scan_dtypes, scan_plan, sort_plan, topk_plan, knn_plan,
                     compact_tile, stencil_plan, potrf_plan, geqr_plan, syevj_plan, gesvj_plan, csrmm_plan, als_plan,
                     apsp_plan, fuzzy_plan, nbody_plan, pairwise_plan, PAIR_METRICS, gemm_plan, GEMM_KERNELS,
                     current_stream, _arr, _check, _k_limit, _ptr)
from .util import prod

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC_PATH = os.path.join(_HERE, 'csrc', 'spx.hip')


def __getattr__(name):
  if name in ('COMPACT_TILE', 'TOPK_K_MAX', 'KNN_K_MAX'):  # read from the library on first use
    return getattr(binding, name)
  raise AttributeError('module %r has no attribute %r' % (__name__, name))


class QrHandle:
  """What ``geqr`` leaves for ``orgqr``: the workspace tensor (reflectors, taus,
  signs) and the geometry it was laid out for."""
  __slots__ = ('workspace', 'm', 'n', 'dtype')

  def __init__(self, workspace, m, n, dtype):
    self.workspace, self.m, self.n, self.dtype = workspace, m, n, dtype


class CsrWorkspace:
  """The cached structure analysis of one CSR tile for ``csrmm``: the workspace
  tensor and whether a call has left the long-row lists in it."""
  __slots__ = ('buf', 'prepared')

  def __init__(self):
    self.buf, self.prepared = None, False


# ------------------------------------------------------------ JIT compile
def clang_path():
  rocm = os.environ.get('ROCM_PATH', '/opt/rocm')
  p = os.path.join(rocm, 'lib', 'llvm', 'bin', 'clang++')
  if not os.path.exists(p):
    raise RuntimeError('device compiler %s not found' % p)
  return p


COMPILE_FLAGS = ['-x', 'hip', '--offload-arch=gfx950', '--cuda-device-only', '--no-gpu-bundle-output',
                 '-nogpuinc', '-O3', '-ffp-contract=off', '-std=c++17']


def cache_dir():
  d = FLAGS.kernel_cache_dir or os.path.join(_HERE, '_kcache')
  try:
    os.makedirs(d, exist_ok=True)
    if os.access(d, os.W_OK):
      return d
  except OSError:
    pass
  d = os.path.join(tempfile.gettempdir(), 'spartan_amd_kcache')
  os.makedirs(d, exist_ok=True)
  return d


def source_key(src):
  h = hashlib.sha1()
  h.update(' '.join(COMPILE_FLAGS).encode())
  h.update(src.encode())
  return h.hexdigest()[:24]


def compile_code_object(src):
  """Compile generated HIP source to a gfx950 code object (cached on disk)."""
  key = source_key(src)
  d = cache_dir()
  path = os.path.join(d, key + '.hsaco')
  if os.path.exists(path):
    with open(path, 'rb') as f:
      return f.read()
  # also look in the in-tree cache when an override dir is used
  intree = os.path.join(_HERE, '_kcache', key + '.hsaco')
  if os.path.exists(intree):
    with open(intree, 'rb') as f:
      return f.read()
  with tempfile.TemporaryDirectory() as td:
    sp = os.path.join(td, 'k.hip')
    op = os.path.join(td, 'k.hsaco')
    with open(sp, 'w') as f:
      f.write(src)
    r = subprocess.run([clang_path()] + COMPILE_FLAGS + ['-o', op, sp], capture_output=True, text=True)
    if r.returncode != 0:
      raise RuntimeError('gfx950 codegen compile failed:\n%s\n--- source ---\n%s' % (r.stderr, src))
    with open(op, 'rb') as f:
      img = f.read()
  tmp = path + '.%d.tmp' % os.getpid()
  with open(tmp, 'wb') as f:
    f.write(img)
  os.replace(tmp, path)
  return img


_NCU = []
MAP_UNROLL = 1  # vectors per lane of a dense map (grid = n / (256 V MAP_UNROLL))
NT_STORE_BYTES = 64 << 20  # map outputs at least this large: non-temporal stores
ROWS_GRID_PER_CU = 2  # rows reductions: 1.824 ms vs 1.836 uncapped at cfg2 axis 1 (profiles/r02_cfg2_grid.txt)
# fused row-dot column reductions (cfg5's gradient): blocks per CU, rows
# unrolled per lane group, and the row order.  Round 5: the blocks take
# interleaved super-chunks of U x 16 rows (block p: chunks p, p + P, ...;
# codegen.gen_reduce interleave) instead of one contiguous chunk each, so the
# grid streams one stretch of X at a time -- and then ONE block per CU is
# best: 3.600 ms per lreg iteration against 3.811 for the round-4 form (16
# contiguous chunks per CU, U 8) on one box; interleaved with 2 / 4 / 8 / 16
# blocks per CU 3.69-3.88, U 4 / 6 / 10 / 12 at one block 5.11 / 3.97 / 3.62
# / 3.71 (tools/lreg_il.py, profiles/r05_lreg_interleave.txt)
ROWDOT_BLOCKS_PER_CU = 1
ROWDOT_UNROLL = 8
ROWDOT_INTERLEAVE = True
# wide column sums (several column tiles: cfg2 axis 0): resident blocks per
# CU and whether their row segments are interleaved super-chunks.  The lreg
# kernel's interleaving does NOT carry over: cfg2 axis 0 ran 1.80 ms
# contiguous at 2 blocks per CU against 1.95-2.00 interleaved at 2 / 4 and
# 2.8-3.1 at one block (tools/cfg2_il.py, profiles/r05_cfg2_interleave.txt)
COLS_BLOCKS_PER_CU = 2
COLS_INTERLEAVE = False
# paired sums (HipBackend.reduce): an axis-0 sum that an axis-1 sum of the
# same tree over the same tensors has followed before also writes per-tile
# row sums, and the following axis-1 sum is served from them without a second
# pass over the inputs (cfg2: one 12.9 GB read per step instead of two).
# PAIR_SUMS: the master switch; PAIR_MIN_BYTES: launches reading less than
# this are never paired (a second pass is cheap, the bookkeeping is not)
PAIR_SUMS = True
PAIR_MIN_BYTES = 64 << 20
PAIR_SEEN_MAX = 256  # pair keys remembered (seen-then-speculate)
PAIR_MEMO_MAX = 16   # row-sum tensors held for a following axis-1 sum
# libspx entry points that take tables of device pointers (addresses the
# pointer scan of _call cannot see): calling one drops every held row sum.
# The binding has one, and HipBackend does not call it today (comm.py does,
# on exchange buffers of its own)
PAIR_TABLE_CALLS = frozenset(['spx_sendrecv'])


def _num_cus():
  if not _NCU:
    import torch
    _NCU.append(torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count)
  return _NCU[0]


# What backend.reduce launches for one operand layout.  kind .. kint: the
# kernel (codegen.gen_reduce's arguments); nblk: the grid (0: empty output,
# nothing to launch); P: partials per output element, n_out of them each, in
# pdt; direct: the kernel writes the result itself (no finalize pass); args:
# the KArgs block with dims, strides, aux, flags and the arg-index geometry
# filled in -- pointers, scalars, out0 / out1 are per call (_run_reduce).
ReducePlan = namedtuple('ReducePlan', 'kind classes V U rowinv klpr kfull kint nblk P n_out arg direct pdt args')


def _lanes(need):
  """Lanes of a wave per segment / row group: the power of two >= need, at most 64."""
  lpr = 1
  while lpr < need and lpr < 64:
    lpr *= 2
  return lpr


def plan_reduce(root, op, ins, res16, view, out_dtype, idx_geom, ncu):
  """The ReducePlan of a fused map+reduce: pure integer arithmetic, no device.
  ins: [(slot, NumPy dtype)] in slot order; res16: per input its pointer's
  residue mod 16 (vec_width keeps V * itemsize <= 16, so the residue decides
  the vector path); view: layout.reduce_view's (O, R, I, per-input strides);
  ncu: the device's CU count.  Reads the module's grid / layout knobs."""
  O, R, I, vstr = view
  n_out = O * I
  arg = op in ('argmin', 'argmax')
  adt = codegen.acc_dtype(op, root.dtype)
  if n_out == 0:
    return ReducePlan(None, (), 1, None, (), None, False, False, 0, 1, 0, arg, True, adt, None)
  if R == 0:
    raise ValueError('zero-size reduction')
  V = codegen.vec_width([dt for _, dt in ins] + [adt])
  rowdot = bool(codegen.rowdots(root))
  # the vectorised dim (R of the (O, R) forms, I of (O, R, I)): its extent, every
  # pointer and a contiguous input's other strides must be multiples of V
  vd, n = (1, R) if I == 1 else (2, I)
  classes = tuple(_cls(st[vd]) for st in vstr)
  vec_ok = V > 1 and n % V == 0 and all(
      res16[k] % (V * np.dtype(dt).itemsize) == 0 and
      (classes[k] != 'c' or all(vstr[k][d] % V == 0 for d in range(3) if d != vd))
      for k, (_, dt) in enumerate(ins))
  per = V if vec_ok else 1
  args = codegen.KArgs()
  for k, (s, _) in enumerate(ins):
    for d in range(3):
      args.str[s][d] = vstr[k][d]
  args.dim[0], args.dim[1], args.dim[2] = O, R, I
  args.flags = 1 if vec_ok else 0
  target_blocks = 2048
  P, lpr, CT = 1, None, None
  if I == 1 and R <= 64 * V * 16:
    # short segments: several per wave (LPR lanes each), grid-stride over O
    kind = 'rowsp'
    lpr = _lanes(-(-R // per))
    seg_per_block = 4 * (64 // lpr)
    nblk = max(1, min(-(-O // seg_per_block), 256 * 16))
    args.aux[0], args.aux[1], args.aux[2] = 1, R, lpr.bit_length() - 1
  elif I == 1:
    kind = 'rows'
    if O < target_blocks:
      P = max(1, min(-(-target_blocks // O), -(-R // (256 * per * 4))))
    chunk = -(-R // P)
    chunk = -(-chunk // per) * per
    P = -(-R // chunk)
    # grid-stride kernel: at most ROWS_GRID_PER_CU resident blocks per CU
    # stream the segments
    nblk = min(O * P, ROWS_GRID_PER_CU * ncu)
    args.aux[0], args.aux[1] = P, chunk
  else:
    kind = 'cols'
    lpr = _lanes(-(-I // per))
    CT = -(-I // (lpr * per))
    rows_per_step = 4 * (64 // lpr)
    base = CT * O
    # wide column reductions (several column tiles) stream best with
    # exactly two resident blocks per CU (cfg2 axis 0: 512 blocks 1.80 ms,
    # 1024 1.87, 2048 1.87, 4096 1.90); one narrow column tile (cfg5's 64
    # columns) with eight (2048: 4.06 ms per lreg iteration, 512: 4.15)
    # -- profiles/r02_cfg2_grid.txt; a fused row dot (cfg5's gradient, one
    # 64-column tile) with ROWDOT_BLOCKS_PER_CU (one, its rows interleaved
    # over the blocks: see ROWDOT_INTERLEAVE)
    tb = (COLS_BLOCKS_PER_CU if CT > 1 else ROWDOT_BLOCKS_PER_CU if rowdot else 8) * ncu
    if base < tb:
      P = max(1, min(-(-tb // base), -(-R // (rows_per_step * 4))))
    chunk = -(-R // P)
    P = -(-R // chunk)
    nblk = base * P
    args.aux[0], args.aux[1], args.aux[2], args.aux[3] = P, chunk, lpr.bit_length() - 1, CT
  if rowdot and (kind != 'cols' or CT != 1):
    raise NotImplementedError('fused row dot needs each row in one lane group (K <= 64 * vector width)')
  if nblk > 0x7fffffff:
    raise NotImplementedError('reduction grid too large')
  if arg:
    g = idx_geom or {}
    args.aux[4] = g.get('offset', 0)
    args.aux[5] = 1 if g.get('decompose') else 0
    if g.get('decompose'):
      tshape, tul, ashape = g['tshape'], g['tul'], g['ashape']
      args.aux[6] = len(tshape)
      for d in range(len(tshape)):
        args.tshape[d], args.tul[d], args.ashape[d] = tshape[d], tul[d], ashape[d]
  U, rowinv, klpr, kfull = None, (), None, False
  if kind == 'cols':
    U = ROWDOT_UNROLL if rowdot else codegen.cols_unroll(ins, classes, V, [st[1] for st in vstr])
    rowinv = tuple(s for (s, _), st in zip(ins, vstr) if st[1] == 0)
    # a fused row dot's lane group width (and whether the vector path covers
    # the columns exactly) is compiled in: its per-row lane sum is then
    # straight-line DPP (codegen.gen_reduce)
    if rowdot:
      klpr, kfull = lpr, bool(vec_ok and I == lpr * per)
  kint = bool((klpr and ROWDOT_INTERLEAVE) or (kind == 'cols' and CT > 1 and op == 'sum' and COLS_INTERLEAVE))
  # partials' dtype: fp64 for an interleaved fp32 sum (codegen.partial_dtype)
  pdt = codegen.partial_dtype(op, adt, kint) if kind == 'cols' else adt
  direct = P == 1 and (arg or pdt == np.dtype(out_dtype))
  return ReducePlan(kind, classes, V, U, rowinv, klpr, kfull, kint, nblk, P, n_out, arg, direct, pdt, args)


def pair_eligible(root, op, ins, view, plan):
  """Whether the launch ``plan`` (plan_reduce's, for ``view``) may run as the
  paired kernel (codegen.gen_reduce pair=True): a floating column sum of one
  (R, I) matrix without row dot or interleaving, on the vector path, whose
  column tiles cover I exactly, that reads at least PAIR_MIN_BYTES.  Pure
  integer arithmetic, no device; reads PAIR_SUMS and PAIR_MIN_BYTES."""
  O, R, I, vstr = view
  if not PAIR_SUMS or plan.kind != 'cols' or op != 'sum' or O != 1 or plan.kint or not plan.args.flags & 1:
    return False
  if not codegen.is_float(codegen.acc_dtype(op, root.dtype)) or codegen.rowdots(root):
    return False
  lpr, CT = 1 << plan.args.aux[2], plan.args.aux[3]
  if I != CT * lpr * plan.V:
    return False
  read = sum(np.dtype(dt).itemsize * (R if st[1] else 1) * (I if st[2] else 1) for (_, dt), st in zip(ins, vstr))
  return read >= PAIR_MIN_BYTES


def _scalar_values(root):
  """The values of a tree's Sc leaves, in walk order."""
  return tuple((n.slot, n.value) for n in codegen.walk(root) if isinstance(n, codegen.Sc))


def _mem_range(t):
  """[first byte, one past the last) of the allocation behind tensor ``t``:
  what any view of the same storage can reach."""
  st = t.untyped_storage()
  return st.data_ptr(), st.data_ptr() + st.nbytes()


class _ClearHooked(dict):
  """A dict whose clear() also calls ``on_clear`` (HipBackend._reduce_plans and
  eval_cache's store: clearing either drops the paired-sum state)."""
  on_clear = None

  def clear(self):
    dict.clear(self)
    if self.on_clear is not None:
      self.on_clear()


_pair_backends = weakref.WeakSet()  # backends whose held row sums an eval_cache.clear() drops


def _drop_all_pair_memos():
  for be in list(_pair_backends):
    be._pair_memo.clear()


def _watch_eval_cache(be):
  """From now on eval_cache.clear() drops ``be``'s held row sums."""
  from .expr.base import eval_cache
  if not isinstance(eval_cache.cache, _ClearHooked):
    eval_cache.cache = _ClearHooked(eval_cache.cache)
    eval_cache.cache.on_clear = _drop_all_pair_memos
  _pair_backends.add(be)


# One held row-sum result: the tensor, weak references to the operand tensors
# it was computed from, their _version counters and allocations, the tree's
# scalar values.
_PairEntry = namedtuple('_PairEntry', 'rows refs versions ranges scalars')
# The previous reduce call when it was an eligible axis-0 sum.
_PairLast = namedtuple('_PairLast', 'key refs scalars')


class HipBackend:
  """Launches libspx.so / generated kernels on the current HIP stream."""
  name = 'hip'

  def __init__(self):
    self.lib = load_library()
    self._fns = {}
    self._modules = []
    self._lock = threading.Lock()
    self.launch_log = None   # optional list collecting grids (tests)
    self.kernel_events = None  # optional list of (name, start, end) HIP events (bench)
    self._names = {}
    self._sig_fns = {}
    self._reduce_plans = _ClearHooked()  # backend.reduce launch plans (see reduce)
    self._reduce_plans.on_clear = self._pair_reset
    # paired sums (see reduce): the pair keys seen, the previous call when it
    # was an eligible axis-0 sum, the held row sums by pair key, and whether
    # the call under way is the paired launch itself
    self._pair_seen = set()
    self._pair_last = None
    self._pair_memo = {}
    self._pair_own = False
    self._fuzzy_ws = {}  # fuzzy_step workspaces by (dtype, D, K, device)
    self._nbody_ws = {}  # nbody_accel workspaces (the float64 partials of a split) by device
    self._pairwise_ws = {}  # pairwise workspaces (the float64 row-sum partials of a split) by device

  # ---------------------------------------------------------------- utils
  def stream(self):
    return current_stream()

  def kernel(self, src, name):
    key = source_key(src)
    with self._lock:
      fn = self._fns.get(key)
      if fn is not None:
        return fn
      img = compile_code_object(src)
      mod = ctypes.c_void_p()
      _check(self.lib.spx_module_load(img, len(img), ctypes.byref(mod)), 'spx_module_load')
      self._modules.append(mod)
      f = ctypes.c_void_p()
      _check(self.lib.spx_module_function(mod, name.encode(), ctypes.byref(f)), 'spx_module_function')
      self._fns[key] = f
      self._names[f.value] = name
      return f

  def _events(self):
    """A (start, end) pair of HIP events, start recorded on the current
    stream, when bench timing is on (kernel_events), else None."""
    if self.kernel_events is None:
      return None
    import torch
    ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
    ev[0].record()
    return ev

  def _call(self, name, *args, timed=True):
    """One ahead-of-time libspx call ``name`` on the current stream, which
    every compute entry point takes last.  ``timed``: between _events(), logged
    under ``name``.  The arguments go to ctypes as they are."""
    if self._pair_memo and not self._pair_own:
      if name in PAIR_TABLE_CALLS:
        self._pair_memo.clear()
      else:
        self._pair_scan([a.value for a in args if isinstance(a, ctypes.c_void_p) and a.value])
    ev = self._events() if timed else None
    if ev is not None:
      self.kernel_events.append((name, ev[0], ev[1]))
    _check(getattr(self.lib, name)(*args, current_stream()), name)
    if ev is not None:
      ev[1].record()

  def _workspace_for(self, query, sizes, device, bad, floor=0, exc=ValueError):
    """(tensor or None, its bytes): the shared scratch buffer of at least
    ``floor`` bytes that the library's ``query`` asks for ``sizes``; ``exc(bad)``
    where it rejects them."""
    need = getattr(self.lib, query)(*sizes)
    if need < 0:
      raise exc(bad)
    need = max(int(need), floor)
    if need == 0:
      return None, 0
    ws = self._workspace(need, device)
    return ws, ws.numel()

  def kmeans_timing(self, enable):
    """Record HIP events around the one-pass kernel of every later fused
    spx_kmeans_step (bench.py's k-means kernel roofline)."""
    _check(self.lib.spx_kmeans_timing(1 if enable else 0), 'spx_kmeans_timing')

  def kmeans_times(self, max_calls=256):
    """[(fused kernel ms, whole step ms)] of the steps recorded since
    kmeans_timing(True) or the last call (waits for them)."""
    a = (ctypes.c_double * max_calls)()
    b = (ctypes.c_double * max_calls)()
    n = self.lib.spx_kmeans_times(a, b, max_calls)
    if n < 0:
      _check(n, 'spx_kmeans_times')
    return [(a[i], b[i]) for i in range(n)]

  def launch(self, fn, grid, args):
    if self.launch_log is not None:
      self.launch_log.append(grid)
    args.grid = grid
    if self._pair_memo and not self._pair_own:
      self._pair_scan([p for p in list(args.ptr) + [args.out0, args.out1] if p])
    ev = self._events()
    _check(self.lib.spx_launch(fn, grid, 1, 1, 256, 0, ctypes.byref(args), ctypes.sizeof(args),
                               current_stream()), 'spx_launch')
    if ev is not None:
      ev[1].record()
      self.kernel_events.append((self._names.get(fn.value, '?'), ev[0], ev[1]))

  # ---------------------------------------------------------------- fills
  def fill(self, out, kind, a, b, seed, ul, array_shape):
    shape = tuple(out.shape)
    nd = len(shape)
    self._call('spx_fill', spx_dtype(np_dtype(out.dtype)), kind, _ptr(out), nd, _arr(shape), _arr(ul),
               _arr(array_shape), float(a), float(b), int(seed) & 0xFFFFFFFFFFFFFFFF, timed=False)

  # ------------------------------------------------------------------ map
  def map(self, root, inputs, out):
    """out[...] = root(inputs) elementwise.  inputs: {slot: tensor} (contiguous,
    broadcastable to out.shape); scalar slots come from the IR's Sc leaves."""
    shape = tuple(out.shape)
    n = prod(shape)
    if n == 0:
      return
    slots = sorted(inputs)
    ins = [(s, np_dtype(inputs[s].dtype)) for s in slots]
    strides = [broadcast_strides(tuple(inputs[s].shape), shape, inputs[s].stride()) for s in slots]
    dense = all(tuple(inputs[s].shape) == shape and inputs[s].is_contiguous() for s in slots)
    V = codegen.vec_width([dt for _, dt in ins] + [root.dtype])
    args = codegen.KArgs()
    _scalars_into(root, args)
    for s in slots:
      args.ptr[s] = inputs[s].data_ptr()
    args.out0 = out.data_ptr()
    args.n = n
    if dense:
      classes = ['c'] * len(slots)
      ndim = 1
      vec_ok = (n % V == 0) and all(inputs[s].data_ptr() % 16 == 0 for s in slots) and out.data_ptr() % 16 == 0
    else:
      cshape, cstr = coalesce(shape, strides)
      ndim = len(cshape)
      if ndim > codegen.MAX_DIM:
        raise NotImplementedError('map over %d non-coalescible dims' % ndim)
      for d in range(ndim):
        args.dim[d] = cshape[d]
      for k, s in enumerate(slots):
        for d in range(ndim):
          args.str[s][d] = cstr[k][d]
      classes = [_cls(cstr[k][ndim - 1]) for k in range(len(slots))]
      vec_ok = (cshape[-1] % V == 0) and out.data_ptr() % 16 == 0 and all(
          _vec_aligned(inputs[s], cstr[k], classes[k], V) for k, s in enumerate(slots))
    args.flags = 1 if (vec_ok and V > 1) else 0
    # streamed outputs: non-temporal stores (x*y+exp(z) map at 2^30 fp32:
    # 2.75 -> 2.57 ms, profiles/r02_stream_ceiling_maps.txt)
    nt = n * out.element_size() >= NT_STORE_BYTES
    mu = MAP_UNROLL if (dense and args.flags & 1) else 1
    sig = ('map', root.sig(), tuple(ins), tuple(classes), ndim, V, dense, nt, mu)
    fn = self._sig_fns.get(sig)
    if fn is None:
      src, kname = codegen.named(codegen.gen_map(root, ins, classes, ndim, V, dense, nt, mu), 'spx_map',
                                 'dense' if dense else 'nd')
      fn = self._sig_fns[sig] = self.kernel(src, kname)
    per = V if args.flags & 1 else 1
    # MAP_UNROLL vectors per lane and no grid-stride loop: x + 1 / x * y at
    # 2^30 fp32 1.75 / 2.58 ms with a 4096-block grid-stride loop, 1.34 / 2.01
    # ms with the full grid (6.4 TB/s read+write; profiles/r02_map_grid.txt)
    grid = max(1, -(-n // (256 * per * mu)))
    self.launch(fn, grid, args)

  # --------------------------------------------------------------- reduce
  def reduce(self, root, op, inputs, in_shape, axis, out_shape, out_dtype, idx_geom=None):
    """Fused map+reduce over one tile -> the tile's partial, a device tensor of
    out_shape and out_dtype; for argmin/argmax a (values, int64 indices) pair."""
    import torch
    if np.dtype(out_dtype) not in binding._DT:
      # int8 / uint8 / int16 results: the finalize pass knows no such type, so
      # reduce into the type's accumulator (int32, sums int64) and narrow that
      # with the identity-cast map (wraps like astype)
      wide = self.reduce(root, op, inputs, in_shape, axis, out_shape, codegen.acc_dtype(op, out_dtype), idx_geom)
      return self.contiguous(wide, out_dtype)
    slots = sorted(inputs)
    # launch plan of an identical call (same IR signature, operand layouts and
    # shapes: an iterative driver's replayed DAG): the view, the plan
    # (plan_reduce) and the kernel are functions of this key
    # (the pointer's residue mod 16, not just 16-byte alignment: the vector
    # width of narrow types needs only 8 or 4 bytes, so two pointers with the
    # same 16-alignment verdict can still differ in what V they allow)
    ikey = tuple((s, inputs[s].dtype, tuple(inputs[s].shape), inputs[s].stride(), inputs[s].data_ptr() % 16)
                 for s in slots)
    pkey = (root.sig(), op, ikey, tuple(in_shape), axis, tuple(out_shape), np.dtype(out_dtype).str,
            None if idx_geom is None else repr(sorted(idx_geom.items())),
            # the module's grid / layout knobs shape the plan too
            (ROWS_GRID_PER_CU, COLS_BLOCKS_PER_CU, COLS_INTERLEAVE, ROWDOT_BLOCKS_PER_CU, ROWDOT_UNROLL,
             ROWDOT_INTERLEAVE, PAIR_SUMS, PAIR_MIN_BYTES))
    # paired sums.  A pair key names a tree over operand layouts (not
    # values).  An eligible axis-0 sum (pair_eligible) followed at once by
    # the axis-1 sum of the same tree over the same tensor objects and scalar
    # values puts the key into _pair_seen; from then on the axis-0 sum of that
    # key runs the paired kernel and holds the row sums (_run_pair), and the
    # axis-1 sum that follows takes them (_pair_take) if nothing has touched
    # the operands since
    last, self._pair_last = self._pair_last, None
    if op == 'sum' and axis == 1 and len(in_shape) == 2 and last is not None:
      got = self._pair_take(last, (root.sig(), ikey, tuple(in_shape)), root, inputs, slots, out_shape, out_dtype)
      if got is not None:
        return got
    entry = self._reduce_plans.get(pkey)
    if entry is None:
      ins = [(s, np_dtype(inputs[s].dtype)) for s in slots]
      strides = [broadcast_strides(tuple(inputs[s].shape), in_shape, inputs[s].stride()) for s in slots]
      view = reduce_view(in_shape, strides, axis)
      if view is None and any(not inputs[s].is_contiguous() for s in slots):
        # a strided view whose dims do not collapse to (O, R, I): make the
        # views dense (identity-map kernel) and reduce those (a call of its
        # own: the plan belongs to the copies' layout, not to this key)
        return self.reduce(root, op, {s: self.contiguous(t) for s, t in inputs.items()}, in_shape, axis,
                           out_shape, out_dtype, idx_geom)
      if view is None:
        # inputs broadcast along different dims of an N-d iteration space (e.g.
        # (N, 1, D) - (1, K, D) reduced over the last axis): the rows of the
        # (O, R, I) form have no single stride.  Materialise the mapped values
        # with the N-d map kernel, then reduce that dense array -- in slabs of a
        # kept dim when the whole iteration space exceeds MATERIALISE_LIMIT bytes.
        if codegen.rowdots(root):
          raise NotImplementedError('row-dot reduction over a non-coalescible view')
        dev = out_device(inputs, slots)
        total = prod(in_shape) * np.dtype(root.dtype).itemsize
        if axis is not None and total > self.MATERIALISE_LIMIT:
          kept = [d for d in range(len(in_shape)) if d != axis and in_shape[d] > 1]
          if kept:
            return self._reduce_slabs(root, op, inputs, tuple(in_shape), axis, tuple(out_shape), out_dtype,
                                      idx_geom, kept[0], dev)
        tmp = torch.empty(tuple(in_shape), dtype=torch_dtype(root.dtype), device=dev)
        self.map(root, inputs, tmp)
        return self.reduce(codegen.In(0, root.dtype), op, {0: tmp}, in_shape, axis, out_shape, out_dtype, idx_geom)
      plan = plan_reduce(root, op, ins, [inputs[s].data_ptr() % 16 for s in slots], view, out_dtype, idx_geom,
                         _num_cus())
      fn = None
      if plan.nblk:
        sig = ('reduce', root.sig(), tuple(ins), plan.classes, plan.kind, op, plan.V, plan.U, plan.rowinv,
               plan.klpr, plan.kfull, plan.kint)
        fn = self._sig_fns.get(sig)
        if fn is None:
          src, kname = codegen.named(codegen.gen_reduce(root, ins, *sig[3:]), 'spx_reduce', plan.kind)
          fn = self._sig_fns[sig] = self.kernel(src, kname)
      pk = None
      if (axis == 0 and len(in_shape) == 2 and np.dtype(out_dtype) == plan.pdt and
          pair_eligible(root, op, ins, view, plan)):
        pk = (root.sig(), ikey, tuple(in_shape))
      if len(self._reduce_plans) >= 512:
        self._reduce_plans.clear()
      entry = self._reduce_plans[pkey] = (plan, fn, out_device(inputs, slots), pk)
    pk = entry[3]
    if pk is not None:
      self._pair_memo.pop(pk, None)  # a new axis-0 sum of the key: what an earlier one left is not taken any more
      self._pair_last = _PairLast(pk, tuple(weakref.ref(inputs[s]) for s in slots), _scalar_values(root))
      if pk in self._pair_seen:
        return self._run_pair(entry, root, inputs, slots, out_shape, out_dtype)
    return self._run_reduce(entry, root, op, inputs, slots, out_shape, out_dtype)

  def _pair_reset(self):
    self._pair_seen.clear()
    self._pair_memo.clear()
    self._pair_last = None

  def _pair_scan(self, ptrs):
    """Drop every held row sum one of whose operand allocations holds one of
    the device addresses ``ptrs`` (the pointer arguments of a call about to be
    made; reads count too).  libspx and the generated kernels write through
    raw pointers, which no tensor's _version sees."""
    for key, e in list(self._pair_memo.items()):
      if any(lo <= p < hi for p in ptrs for lo, hi in e.ranges):
        self._pair_memo.pop(key, None)

  def _pair_take(self, last, key, root, inputs, slots, out_shape, out_dtype):
    """An axis-1 sum with pair key ``key`` right after the eligible axis-0 sum
    ``last``.  When the two are one tree over the same tensor objects and
    scalar values the key is noted as seen, and the row sums that the axis-0
    call left (if it ran paired) are returned if they are still those of these
    operands -- handed over once: the entry goes.  Else None."""
    scalars = _scalar_values(root)
    if not (last.key == key and last.scalars == scalars and len(last.refs) == len(slots) and
            all(r() is inputs[s] for r, s in zip(last.refs, slots))):
      return None
    if len(self._pair_seen) >= PAIR_SEEN_MAX:
      self._pair_seen.clear()
    self._pair_seen.add(key)
    e = self._pair_memo.get(key)
    if e is None:
      return None
    if not (e.scalars == scalars and len(e.refs) == len(slots) and
            all(r() is inputs[s] and inputs[s]._version == v for r, v, s in zip(e.refs, e.versions, slots)) and
            tuple(e.rows.shape) == tuple(out_shape) and e.rows.dtype == torch_dtype(out_dtype)):
      return None
    del self._pair_memo[key]
    return e.rows

  def _pair_hold(self, key, rows, root, inputs, slots):
    """Hold ``rows`` for the axis-1 sum that follows the paired launch."""
    memo = self._pair_memo
    while len(memo) >= PAIR_MEMO_MAX:
      del memo[next(iter(memo))]
    drop = lambda _r, memo=memo, key=key: memo.pop(key, None)  # an operand died
    ts = [inputs[s] for s in slots]
    memo[key] = _PairEntry(rows, tuple(weakref.ref(t, drop) for t in ts), tuple(t._version for t in ts),
                           tuple(_mem_range(t) for t in ts), _scalar_values(root))
    _watch_eval_cache(self)

  def _run_pair(self, entry, root, inputs, slots, out_shape, out_dtype):
    """The paired launch of a planned axis-0 sum: the plan's grid and argument
    block, the paired kernel, both partial sets through
    spx_reduce_finalize_pair; returns the column sums and holds the row
    sums."""
    import torch
    p, _, dev, key = entry
    R, CT, lpr = p.args.dim[1], p.args.aux[3], 1 << p.args.aux[2]
    ins = tuple((s, np_dtype(inputs[s].dtype)) for s in slots)
    sig = ('reduce_pair', root.sig(), ins, p.classes, p.V, p.U, p.rowinv, lpr)
    fn = self._sig_fns.get(sig)
    if fn is None:
      src, kname = codegen.named(codegen.gen_reduce(root, list(ins), p.classes, 'cols', 'sum', p.V, p.U, p.rowinv, lpr,
                                                    True, False, pair=True), 'spx_reduce', 'pair')
      fn = self._sig_fns[sig] = self.kernel(src, kname)
    tdt = torch_dtype(p.pdt)
    cols = torch.empty(tuple(out_shape), dtype=tdt, device=dev)
    rows = torch.empty((R,), dtype=tdt, device=dev)
    part_c = torch.empty((p.P * p.n_out,), dtype=tdt, device=dev)
    part_r = torch.empty((CT * R,), dtype=tdt, device=dev)
    args = codegen.KArgs.from_buffer_copy(p.args)
    _scalars_into(root, args)
    for s in slots:
      args.ptr[s] = inputs[s].data_ptr()
    args.out0, args.out1 = part_c.data_ptr(), part_r.data_ptr()
    self._pair_own = True  # these two calls read the operands of held row sums: no scan
    try:
      self.launch(fn, p.nblk, args)
      self._call('spx_reduce_finalize_pair', spx_dtype(p.pdt), _ptr(part_c), p.P, p.n_out, _ptr(cols), _ptr(part_r),
                 CT, R, _ptr(rows), timed=False)
    finally:
      self._pair_own = False
    self._pair_hold(key, rows, root, inputs, slots)
    return cols

  def _run_reduce(self, entry, root, op, inputs, slots, out_shape, out_dtype):
    """Launch a planned reduction (first call and replay alike): the plan's
    kernel, grid and argument block with this call's scalars, pointers and
    output buffers, then the finalize pass over the P partials."""
    import torch
    p, fn, dev = entry[:3]
    tpdt = torch_dtype(p.pdt)  # (arg ops: the values' dtype, pdt == the accumulator's)
    out_shape = tuple(out_shape)
    if p.arg:
      res_v = torch.empty(out_shape, dtype=tpdt, device=dev)
      result = torch.empty(out_shape, dtype=torch.int64, device=dev)
    else:
      res_v, result = None, torch.empty(out_shape, dtype=torch_dtype(out_dtype), device=dev)
    if p.nblk == 0:  # empty output
      return (res_v, result) if p.arg else result
    args = codegen.KArgs.from_buffer_copy(p.args)
    _scalars_into(root, args)
    for s in slots:
      args.ptr[s] = inputs[s].data_ptr()
    if p.direct:
      part_v, part_i = (res_v, result) if p.arg else (result, None)
    else:
      part_v = torch.empty((p.P * p.n_out,), dtype=tpdt, device=dev)
      part_i = torch.empty((p.P * p.n_out,), dtype=torch.int64, device=dev) if p.arg else None
    args.out0 = part_v.data_ptr()
    args.out1 = part_i.data_ptr() if p.arg else 0
    self.launch(fn, p.nblk, args)
    if not p.direct:
      self._finalize(op, p.pdt, np.int64 if p.arg else out_dtype, part_v, part_i, p.P, p.n_out, result, res_v)
    return (res_v, result) if p.arg else result

  def contiguous(self, t, dtype=None):
    """Dense copy of a strided view (and/or dtype conversion) by the generated
    identity-map kernel; ``t`` itself when nothing is to be done."""
    import torch
    src_dt = np_dtype(t.dtype)
    dst_dt = np.dtype(dtype) if dtype is not None else src_dt
    if t.is_contiguous() and dst_dt == src_dt:
      return t
    out = torch.empty(tuple(t.shape), dtype=torch_dtype(dst_dt), device=t.device)
    if t.numel() == 0:
      return out
    root = codegen.In(0, src_dt)
    if dst_dt != src_dt:
      root = codegen.Cast(root, dst_dt)
    self.map(root, {0: t}, out)
    return out

  # ------------------------------------------------------------ finalize
  def finalize(self, op, parts, P, n, out):
    """out[i] = fold over p < P of parts[p * n + i] in p order (sum / min /
    max; NaN propagates for min / max like np.minimum / np.maximum)."""
    self._finalize(op, np_dtype(parts.dtype), np_dtype(out.dtype), parts, None, P, n, out, None)

  def _finalize(self, op, pdt, odt, parts, parts_i, P, n, out, out_v):
    """spx_reduce_finalize: ``parts`` (dtype pdt; arg ops: values, with their
    indices ``parts_i``) -> ``out`` (dtype odt; arg ops: the indices, values
    to ``out_v``)."""
    self._call('spx_reduce_finalize', OP_CODE[op], spx_dtype(pdt), spx_dtype(odt), _ptr(parts), _ptr(parts_i), P, n,
               _ptr(out), _ptr(out_v), timed=False)

  def argcombine(self, op, vals, idx):
    """vals/idx: [R, n] -> (val[n], idx[n]) best-of-R with first-index ties."""
    import torch
    R, n = vals.shape[0], vals.shape[1] if vals.dim() > 1 else 1
    out_i = torch.empty((n,), dtype=torch.int64, device=vals.device)
    out_v = torch.empty((n,), dtype=vals.dtype, device=vals.device)
    self._call('spx_argreduce_combine', OP_CODE[op], spx_dtype(np_dtype(vals.dtype)), _ptr(vals), _ptr(idx), R, n,
               _ptr(out_v), _ptr(out_i), timed=False)
    return out_v, out_i

  # ---------------------------------------------------------------- merge
  def merge(self, dst, mask, region_ul, src, op, fastpath=True):
    shape = tuple(dst.shape)
    self._call('spx_merge', OP_CODE[op], spx_dtype(np_dtype(dst.dtype)), _ptr(dst), _ptr(mask), len(shape),
               _arr(shape), _arr(region_ul), _arr(tuple(src.shape) if src.dim() else ()), _ptr(src),
               spx_dtype(np_dtype(src.dtype)), 1 if fastpath else 0, timed=False)

  def copy_region(self, dst, dst_ul, src, src_ul, shape):
    nd = len(shape)
    self._call('spx_copy_region', spx_dtype(np_dtype(dst.dtype)), _ptr(dst), _arr(tuple(dst.shape)), _arr(dst_ul),
               spx_dtype(np_dtype(src.dtype)), _ptr(src), _arr(tuple(src.shape)), _arr(src_ul), nd, _arr(shape),
               timed=False)

  MATERIALISE_LIMIT = 2 << 30  # bytes of one materialised slab (non-coalescible reductions)

  def _reduce_slabs(self, root, op, inputs, in_shape, axis, out_shape, out_dtype, idx_geom, d, dev):
    """reduce() over slabs of the kept dim ``d`` (each slab materialised and
    reduced on its own), results copied into place."""
    import torch
    nd = len(in_shape)
    per = prod(in_shape) // in_shape[d] * np.dtype(root.dtype).itemsize
    nc = max(1, self.MATERIALISE_LIMIT // max(1, per))
    od = d if d < axis else d - 1  # the same dim in the output
    arg = op in ('argmin', 'argmax')
    res_v = res_i = None
    for c0 in range(0, in_shape[d], nc):
      c1 = min(in_shape[d], c0 + nc)
      sub = {}
      for sl, t in inputs.items():
        td = d - (nd - t.dim())  # inputs broadcast from the right
        sub[sl] = t.narrow(td, c0, c1 - c0) if td >= 0 and t.shape[td] == in_shape[d] else t
      sshape = in_shape[:d] + (c1 - c0,) + in_shape[d + 1:]
      soshape = out_shape[:od] + (c1 - c0,) + out_shape[od + 1:]
      got = self.reduce(root, op, sub, sshape, axis, soshape, out_dtype, idx_geom)
      ul = tuple(c0 if k == od else 0 for k in range(len(out_shape)))
      parts = got if arg else (got,)
      if res_v is None:
        res_v = torch.empty(out_shape, dtype=parts[0].dtype, device=dev)
        if arg:
          res_i = torch.empty(out_shape, dtype=parts[1].dtype, device=dev)
      self.copy_region(res_v, ul, parts[0], (0,) * len(out_shape), soshape)
      if arg:
        self.copy_region(res_i, ul, parts[1], (0,) * len(out_shape), soshape)
    return (res_v, res_i) if arg else res_v

  # ----------------------------------------------------------------- gemm
  def gemm(self, A, B, C, alpha=1.0, beta=0.0):
    """C = alpha * A @ B + beta * C for 2-d contiguous row-major tensors."""
    M, K = A.shape
    K2, N = B.shape
    assert K == K2 and tuple(C.shape) == (M, N)
    dt = np_dtype(A.dtype)
    self._call('spx_gemm', spx_dtype(dt), M, N, K, _ptr(A), A.stride(0), _ptr(B), B.stride(0), _ptr(C), C.stride(0),
               float(alpha), float(beta))

  # --------------------------------------------------------------- k-means
  def kmeans_assign(self, points, centers, labels, mindist=None, exact_only=False, dist_dtype=np.float64):
    """labels[p] = first argmin_c cdist(points[p], centers[c]) (exact fp64
    order; dist_dtype float32: of the distances rounded to fp32).  Default:
    MFMA-certified fast path + exact-order kernel for the undecided points;
    exact_only=True (or mindist) runs every point exactly."""
    N, D = points.shape
    K = centers.shape[0]
    assert centers.dtype == self._f64() and tuple(centers.shape) == (K, D) and labels.shape[0] == N
    dt = spx_dtype(np_dtype(points.dtype))
    ws, nws = None, 0
    if mindist is None and not exact_only and N > 0:
      ws, nws = self._workspace_for('spx_kmeans_assign_workspace', (dt, N, D, K), points.device,
                                    'spx_kmeans_assign_workspace: bad arguments', exc=RuntimeError)
    self._call('spx_kmeans_assign', dt, N, D, K, _ptr(points), points.stride(0), _ptr(centers), _ptr(labels),
               _ptr(mindist), _ptr(ws), nws, spx_dtype(dist_dtype), timed=False)

  def kmeans_accumulate(self, points, labels, sums, counts, zero_first=True):
    N, D = points.shape
    K = sums.shape[0]
    dt = spx_dtype(np_dtype(points.dtype))
    ws, nws = self._workspace_for('spx_kmeans_accumulate_workspace', (dt, N, D, K), points.device,
                                  'spx_kmeans_accumulate_workspace: bad arguments', floor=8, exc=RuntimeError)
    self._call('spx_kmeans_accumulate', dt, N, D, K, _ptr(points), points.stride(0), _ptr(labels), _ptr(sums),
               _ptr(counts), 1 if zero_first else 0, _ptr(ws), nws, timed=False)

  def kmeans_step(self, points, centers, labels, sums, counts, zero_first=True, dist_dtype=np.float64):
    """kmeans_assign + kmeans_accumulate in one call (spx_kmeans_step): the
    certified screen labels and accumulates the decided rows in one pass."""
    N, D = points.shape
    K = centers.shape[0]
    assert centers.dtype == self._f64() and tuple(centers.shape) == (K, D) and labels.shape[0] == N
    assert tuple(sums.shape) == (K, D) and counts.shape[0] == K and sums.is_contiguous() and counts.is_contiguous()
    dt = spx_dtype(np_dtype(points.dtype))
    ws, nws = self._workspace_for('spx_kmeans_step_workspace', (dt, N, D, K), points.device,
                                  'spx_kmeans_step_workspace: bad arguments', floor=8, exc=RuntimeError)
    self._call('spx_kmeans_step', dt, N, D, K, _ptr(points), points.stride(0), _ptr(centers), _ptr(labels),
               _ptr(sums), _ptr(counts), 1 if zero_first else 0, _ptr(ws), nws, spx_dtype(dist_dtype), timed=False)

  def cdist(self, points, centers, out):
    """out (N, K) = exact-order cdist(points, centers), rounded to out's dtype."""
    N, D = points.shape
    K = centers.shape[0]
    assert centers.dtype == self._f64() and tuple(centers.shape) == (K, D) and tuple(out.shape) == (N, K)
    assert centers.is_contiguous() and points.stride(1) == 1 and out.stride(1) == 1
    self._call('spx_cdist', spx_dtype(np_dtype(points.dtype)), spx_dtype(np_dtype(out.dtype)), N, D, K, _ptr(points),
               points.stride(0), _ptr(centers), _ptr(out), out.stride(0), timed=False)

  def bincount(self, labels, counts, zero_first=True):
    """counts (K,) int64 (+)= bincount of int64 ``labels`` (out-of-range skipped)."""
    assert labels.dtype == counts.dtype and labels.is_contiguous() and counts.is_contiguous()
    self._call('spx_bincount', _ptr(labels), labels.numel(), counts.numel(), _ptr(counts), 1 if zero_first else 0,
               timed=False)

  # ----------------------------------------------------------------- scan
  def scan(self, src, out, axis_geom, carry=None, totals=None, exclusive=False):
    """Cumulative sum of the contiguous tensor ``src`` viewed as (outer, n,
    inner) = ``axis_geom`` along n (spx_scan).  ``out`` (np.cumsum's dtype for
    src's) may be None for a totals-only pass; ``carry`` / ``totals`` are
    contiguous (outer, inner) tensors in the accumulator dtype (int64 /
    float64): carry is added to every element of its line, totals receives
    each line's inclusive total without the carry.  exclusive: out[i] = carry
    + the sum before i.  Asynchronous on the current stream."""
    outer, n, inner = (int(v) for v in axis_geom)
    dt = np_dtype(src.dtype)
    odt, adt = scan_dtypes(dt)
    if not src.is_contiguous() or src.numel() != outer * n * inner:
      raise ValueError('scan: src must be contiguous with %d elements' % (outer * n * inner))
    if out is not None:
      _dense('scan: out', out, odt, src.numel(), 'src\'s size')
    for name, t in (('carry', carry), ('totals', totals)):
      if t is not None:
        _dense('scan: %s' % name, t, adt, outer * inner, '%d elements' % (outer * inner))
    ws, nws = self._workspace_for('spx_scan_workspace', (spx_dtype(dt), outer, n, inner), src.device,
                                  'scan: bad geometry %s' % (axis_geom,))
    self._call('spx_scan', spx_dtype(dt), _ptr(src), _ptr(out), outer, n, inner, _ptr(carry), _ptr(totals),
               1 if exclusive else 0, _ptr(ws), nws)

  # ----------------------------------------------------------------- sort
  def sort(self, src, out_vals, out_idx, axis_geom):
    """Stable ascending sort of the contiguous tensor ``src`` viewed as
    (outer, n, inner) = ``axis_geom`` along n (spx_sort), in NumPy's order
    (NaNs last, -0.0 == +0.0).  ``out_vals`` (src's dtype) receives the
    sorted values, ``out_idx`` (int64) the positions within the line --
    np.argsort(kind='stable'); either may be None, not both, and neither may
    be ``src``.  Asynchronous on the current stream."""
    outer, n, inner = (int(v) for v in axis_geom)
    dt = np_dtype(src.dtype)
    if not src.is_contiguous() or src.numel() != outer * n * inner:
      raise ValueError('sort: src must be contiguous with %d elements' % (outer * n * inner))
    if out_vals is None and out_idx is None:
      raise ValueError('sort: out_vals and out_idx are both None')
    for name, t, odt in (('out_vals', out_vals, dt), ('out_idx', out_idx, np.dtype(np.int64))):
      if t is None:
        continue
      _dense('sort: %s' % name, t, odt, src.numel(), 'src\'s size')
      if src.numel() and t.data_ptr() == src.data_ptr():
        raise ValueError('sort: %s may not be src' % name)
    ws, nws = self._workspace_for('spx_sort_workspace',
                                  (spx_dtype(dt), outer, n, inner, 1 if out_idx is not None else 0), src.device,
                                  'sort: bad geometry %s' % (axis_geom,))
    if src.numel() == 0:
      return
    self._call('spx_sort', spx_dtype(dt), _ptr(src), _ptr(out_vals), _ptr(out_idx), outer, n, inner, _ptr(ws), nws)

  # ----------------------------------------------------------------- topk
  def topk(self, src, in_idx, out_vals, out_idx, axis_geom, k, largest=False):
    """The first ``k`` of each line's stable order (spx_topk): ``src`` is a
    contiguous tensor viewed as (outer, n, inner) = ``axis_geom``; the outputs
    are contiguous with outer * k * inner elements.  ``largest``: descending,
    equal keys lower position first, NaNs still last.  ``out_vals`` (src's
    dtype) receives the selected values, ``out_idx`` (int64) their positions
    in the line or, with ``in_idx`` (int64, src's size), in_idx there; either
    output may be None, not both.  Asynchronous on the current stream."""
    outer, n, inner = (int(v) for v in axis_geom)
    k = int(k)
    dt = np_dtype(src.dtype)
    i64 = np.dtype(np.int64)
    if not src.is_contiguous() or src.numel() != outer * n * inner:
      raise ValueError('topk: src must be contiguous with %d elements' % (outer * n * inner))
    if out_vals is None and out_idx is None:
      raise ValueError('topk: out_vals and out_idx are both None')
    if k < 1 or (outer * inner > 0 and k > n):
      raise ValueError('topk: k %d is outside [1, %d]' % (k, n))
    if k > _k_limit('TOPK_K_MAX'):
      raise ValueError('topk: k %d exceeds TOPK_K_MAX = %d' % (k, _k_limit('TOPK_K_MAX')))
    if in_idx is not None:
      _dense('topk: in_idx', in_idx, i64, src.numel(), 'src\'s size')
    for name, t, odt in (('out_vals', out_vals, dt), ('out_idx', out_idx, i64)):
      if t is None:
        continue
      _dense('topk: %s' % name, t, odt, outer * k * inner, '%d elements' % (outer * k * inner))
      if src.numel() and t.data_ptr() == src.data_ptr():
        raise ValueError('topk: %s may not be src' % name)
    ws, nws = self._workspace_for('spx_topk_workspace',
                                  (spx_dtype(dt), outer, n, inner, k, 1 if out_idx is not None else 0), src.device,
                                  'topk: bad geometry %s, k %d' % (axis_geom, k))
    if outer * inner == 0:
      return
    self._call('spx_topk', spx_dtype(dt), _ptr(src), _ptr(in_idx), _ptr(out_vals), _ptr(out_idx), outer, n, inner, k,
               1 if largest else 0, _ptr(ws), nws)

  def knn(self, points, queries, k, index_base, out_s, out_idx):
    """The k nearest of ``points`` (N, D) float32 / float64, unit column
    stride, to each row of ``queries`` (Q, D) float64 contiguous (spx_knn):
    ``out_s`` (Q, k) float64 receives the exact-order sums of squared
    differences, ascending by (sum, index), ``out_idx`` (Q, k) int64
    index_base + the point's row.  Asynchronous on the current stream."""
    k = int(k)
    if points.dim() != 2 or queries.dim() != 2 or points.shape[1] != queries.shape[1]:
      raise ValueError('knn: points (N, D) and queries (Q, D) expected, got %s and %s'
                       % (tuple(points.shape), tuple(queries.shape)))
    N, D = (int(v) for v in points.shape)
    Q = int(queries.shape[0])
    dt = np_dtype(points.dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
      raise ValueError('knn: points must be float32 / float64, not %s' % dt)
    if queries.dtype != self._f64() or not queries.is_contiguous():
      raise ValueError('knn: queries must be a contiguous float64 tensor')
    if D < 1 or (N > 1 and points.stride(1) != 1) or (N > 1 and points.stride(0) < D):
      raise ValueError('knn: points need unit column stride and a row stride of at least D')
    if k < 1 or k > N:
      raise ValueError('knn: k %d is outside [1, N = %d]' % (k, N))
    if k > _k_limit('KNN_K_MAX'):
      raise ValueError('knn: k %d exceeds KNN_K_MAX = %d' % (k, _k_limit('KNN_K_MAX')))
    for name, t, odt in (('out_s', out_s, np.dtype(np.float64)), ('out_idx', out_idx, np.dtype(np.int64))):
      if np_dtype(t.dtype) != odt or not t.is_contiguous() or tuple(t.shape) != (Q, k):
        raise ValueError('knn: %s must be a contiguous (%d, %d) %s tensor' % (name, Q, k, odt))
    ws, nws = self._workspace_for('spx_knn_workspace', (spx_dtype(dt), Q, N, D, k), points.device,
                                  'knn: bad arguments (Q %d, N %d, D %d, k %d)' % (Q, N, D, k), floor=8)
    if Q == 0:
      return
    ldp = int(points.stride(0)) if N > 1 else D
    self._call('spx_knn', spx_dtype(dt), Q, N, D, k, _ptr(points), ldp, _ptr(queries), int(index_base), _ptr(out_s),
               _ptr(out_idx), _ptr(ws), nws)

  # ------------------------------------------------------- take / compress
  def take(self, src, idx, out, geom, lo, n_total, out_strides=None):
    """out[o, j, :] = src[o, idx[j] - lo, :] (spx_take).  ``src`` is the
    contiguous block ``geom`` = (outer, n_local, inner) holding rows [lo, lo +
    n_local) of an axis of length ``n_total``; ``idx`` a contiguous 1-d int32 /
    int64 tensor of m indices, negative ones wrapped by n_total.  ``out``
    (src's dtype, contiguous) is addressed from its first element by
    ``out_strides`` = (outer stride, row stride) in elements -- default the
    dense (m * inner, inner) -- and rows whose index falls outside [lo, lo +
    n_local) are left untouched.  An index outside [-n_total, n_total) raises
    IndexError (the device flag is read back: the call waits for the
    kernel); nothing is read or written for it."""
    import torch
    outer, n_local, inner = (int(v) for v in geom)
    lo, n_total = int(lo), int(n_total)
    dt = np_dtype(src.dtype)
    if not src.is_contiguous() or src.numel() != outer * n_local * inner or min(outer, n_local, inner) < 0:
      raise ValueError('take: src must be contiguous with %d elements' % (outer * n_local * inner))
    if idx.dim() != 1 or not idx.is_contiguous() or np_dtype(idx.dtype) not in (np.dtype(np.int32), np.dtype(np.int64)):
      raise ValueError('take: idx must be a contiguous 1-d int32 / int64 tensor')
    if lo < 0 or n_total < 0 or lo + n_local > n_total:
      raise ValueError('take: rows [%d, %d) are not inside an axis of length %d' % (lo, lo + n_local, n_total))
    m = idx.numel()
    oos, ors = (m * inner, inner) if out_strides is None else (int(v) for v in out_strides)
    if out.dtype != src.dtype or not out.is_contiguous():
      raise ValueError('take: out must be a contiguous %s tensor' % dt)
    if outer == 0 or m == 0 or inner == 0:
      return
    if ors < inner or (outer > 1 and oos < inner) or (outer - 1) * oos + (m - 1) * ors + inner > out.numel():
      raise ValueError('take: out of %d elements does not hold strides (%d, %d) of %d x %d rows of %d'
                       % (out.numel(), oos, ors, outer, m, inner))
    if out.data_ptr() == src.data_ptr() and src.numel():
      raise ValueError('take: out may not be src')
    err = torch.empty((1,), dtype=torch.int32, device=src.device)
    self._call('spx_take', spx_dtype(dt), spx_dtype(np_dtype(idx.dtype)), _ptr(src), _ptr(idx), _ptr(out), outer,
               n_total, lo, n_local, m, inner, oos, ors, _ptr(err))
    if int(err.item()):
      raise IndexError('take: an index is out of bounds for an axis of length %d' % n_total)

  def compact_count(self, mask):
    """(total, workspace) of the contiguous bool / uint8 tensor ``mask``
    (spx_compact_count): the number of nonzero bytes, read back from the
    device (the call waits), and the workspace with the scanned tile table
    that ``compact`` with the same mask needs."""
    import torch
    if not mask.is_contiguous() or mask.element_size() != 1:
      raise ValueError('compact_count: mask must be a contiguous bool / uint8 tensor')
    n = mask.numel()
    if n == 0:
      return 0, None
    need = int(self.lib.spx_compact_workspace(n))
    if need < 0:
      raise ValueError('compact_count: bad length %d' % n)
    buf = torch.empty((need + 8,), dtype=torch.uint8, device=mask.device)  # the workspace and the total's word
    self._call('spx_compact_count', _ptr(mask), n, _ptr(buf[need:]), _ptr(buf), need)
    return int(buf[need:].view(torch.int64).item()), buf[:need]

  def compact(self, src, mask, out, geom, workspace):
    """out[o, k, :] = src[o, j_k, :] for the k-th nonzero byte j_k of ``mask``
    (spx_compact).  ``src`` is the contiguous block ``geom`` = (outer, n,
    inner), ``mask`` the n bytes ``compact_count`` saw and ``workspace`` what
    it returned; ``out`` is the dense (outer, total, inner) block of src's
    dtype.  Asynchronous on the current stream."""
    outer, n, inner = (int(v) for v in geom)
    dt = np_dtype(src.dtype)
    if not src.is_contiguous() or src.numel() != outer * n * inner or min(outer, n, inner) < 0:
      raise ValueError('compact: src must be contiguous with %d elements' % (outer * n * inner))
    if not mask.is_contiguous() or mask.element_size() != 1 or mask.numel() != n:
      raise ValueError('compact: mask must be a contiguous bool / uint8 tensor of %d bytes' % n)
    if out.dtype != src.dtype or not out.is_contiguous():
      raise ValueError('compact: out must be a contiguous %s tensor' % dt)
    lines = outer * inner
    if lines == 0 or n == 0:
      if out.numel():
        raise ValueError('compact: out must be empty')
      return
    if out.numel() % lines or out.numel() // lines > n:
      raise ValueError('compact: out of %d elements is not (outer, count, inner) with count <= %d' % (out.numel(), n))
    count = out.numel() // lines
    if count == 0:
      return
    need = int(self.lib.spx_compact_workspace(n))
    if workspace is None or workspace.numel() < need or workspace.element_size() != 1:
      raise ValueError('compact: the workspace of compact_count(mask) is needed (%d bytes)' % need)
    if out.data_ptr() == src.data_ptr():
      raise ValueError('compact: out may not be src')
    self._call('spx_compact', spx_dtype(dt), _ptr(src), _ptr(mask), _ptr(out), outer, n, inner, count,
               _ptr(workspace), workspace.numel())

  # ------------------------------------------------------ stencil / maxpool
  def stencil(self, images, filters, out):
    """out[n, f, x, y] = sum over c, i, j with x + i < W, y + j < H of
    images[n, c, x + i, y + j] * filters[f, c, i, j] (spx_stencil).  All three
    are contiguous 4-d tensors of one dtype, float32 or float64: images (N, C,
    W, H), filters (F, C, fw, fh), out (N, F, W, H).  Asynchronous on the
    current stream."""
    dt = np_dtype(images.dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
      raise TypeError('stencil: dtype %s has no stencil kernel (float32 / float64)' % dt)
    if filters.dtype != images.dtype or out.dtype != images.dtype:
      raise TypeError('stencil: images, filters and out must share one dtype (%s, %s, %s)'
                      % (dt, np_dtype(filters.dtype), np_dtype(out.dtype)))
    if images.dim() != 4 or filters.dim() != 4 or out.dim() != 4:
      raise ValueError('stencil: images, filters and out must be 4-d')
    N, C, W, H = (int(v) for v in images.shape)
    F, fc, fw, fh = (int(v) for v in filters.shape)
    if fc != C:
      raise ValueError('stencil: images have %d channels, filters %d' % (C, fc))
    if min(C, W, H, F, fw, fh) < 1:
      raise ValueError('stencil: empty extent (images %s, filters %s)' % (tuple(images.shape), tuple(filters.shape)))
    if tuple(out.shape) != (N, F, W, H):
      raise ValueError('stencil: out must have shape %s, not %s' % ((N, F, W, H), tuple(out.shape)))
    if not (images.is_contiguous() and filters.is_contiguous() and out.is_contiguous()):
      raise ValueError('stencil: images, filters and out must be contiguous')
    if N == 0:
      return
    if out.data_ptr() in (images.data_ptr(), filters.data_ptr()):
      raise ValueError('stencil: out may not be an input')
    self._call('spx_stencil', spx_dtype(dt), _ptr(images), _ptr(filters), _ptr(out), N, C, W, H, F, fw, fh)

  def maxpool(self, src, out, pool_size, stride):
    """out[n, c, p, q] = max over i, j < pool_size with p stride + i < W and
    q stride + j < H of src[n, c, p stride + i, q stride + j] (spx_maxpool).
    ``src`` is a contiguous (N, C, W, H) tensor of any of the five dtypes,
    ``out`` the contiguous (N, C, ceil(W / stride), ceil(H / stride)) tensor
    of the same dtype.  NaN propagates as in np.maximum.  Asynchronous on the
    current stream."""
    pool_size, stride = int(pool_size), int(stride)
    if pool_size < 1 or stride < 1:
      raise ValueError('maxpool: pool_size %d and stride %d must be at least 1' % (pool_size, stride))
    dt = np_dtype(src.dtype)
    if out.dtype != src.dtype:
      raise TypeError('maxpool: out must have src\'s dtype %s' % dt)
    if src.dim() != 4 or out.dim() != 4:
      raise ValueError('maxpool: src and out must be 4-d')
    N, C, W, H = (int(v) for v in src.shape)
    if min(C, W, H) < 1:
      raise ValueError('maxpool: empty extent %s' % (tuple(src.shape),))
    want = (N, C, -(-W // stride), -(-H // stride))
    if tuple(out.shape) != want:
      raise ValueError('maxpool: out must have shape %s, not %s' % (want, tuple(out.shape)))
    if not (src.is_contiguous() and out.is_contiguous()):
      raise ValueError('maxpool: src and out must be contiguous')
    if N == 0:
      return
    if out.data_ptr() == src.data_ptr():
      raise ValueError('maxpool: out may not be src')
    self._call('spx_maxpool', spx_dtype(dt), _ptr(src), _ptr(out), N * C, W, H, pool_size, stride)

  # --------------------------------------------- cholesky / triangular solve
  @staticmethod
  def _matrix(name, t, rows=None, cols=None, dtype=None):
    """(rows, cols, leading dimension) of a 2-d float32 / float64 tensor with
    unit column stride and a row stride of at least its row length."""
    if t.dim() != 2:
      raise ValueError('%s must be 2-d, got shape %s' % (name, tuple(t.shape)))
    dt = np_dtype(t.dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
      raise ValueError('%s must be float32 / float64, not %s' % (name, dt))
    if dtype is not None and dt != dtype:
      raise ValueError('%s has dtype %s, expected %s' % (name, dt, dtype))
    r, c = (int(v) for v in t.shape)
    if (rows is not None and r != rows) or (cols is not None and c != cols):
      raise ValueError('%s has shape %s, expected (%s, %s)' % (name, (r, c), rows, cols))
    if (c > 1 and t.stride(1) != 1) or (r > 1 and t.stride(0) < c):
      raise ValueError('%s needs unit column stride and a row stride of at least %d' % (name, c))
    return r, c, (int(t.stride(0)) if r > 1 else max(c, 1))

  def potrf(self, A, L):
    """``L`` = the lower Cholesky factor of the square ``A`` (spx_potrf): only
    A's lower triangle is read, L's strict upper triangle becomes +0.0, ``L``
    may be ``A``.  Returns the one-element int32 device tensor ``info`` (0, or
    the order of the first leading minor that is not positive definite);
    nothing here reads it.  Asynchronous on the current stream."""
    import torch
    n, c, lda = self._matrix('potrf: A', A)
    if n != c:
      raise ValueError('potrf: A must be square, got %s' % ((n, c),))
    dt = np_dtype(A.dtype)
    _, _, ldl = self._matrix('potrf: L', L, n, n, dt)
    if n and L.data_ptr() == A.data_ptr() and lda != ldl:
      raise ValueError('potrf: in place needs the same row stride')
    info = torch.zeros((1,), dtype=torch.int32, device=A.device)
    ws, nws = self._workspace_for('spx_potrf_workspace', (spx_dtype(dt), n), A.device, 'potrf: bad size %d' % n)
    if n == 0:
      return info
    self._call('spx_potrf', spx_dtype(dt), n, _ptr(A), lda, _ptr(L), ldl, _ptr(info), _ptr(ws), nws)
    return info

  def trsm(self, L, B, side='L', trans=False):
    """Solve with the lower-triangular, non-unit ``L`` in place on ``B`` (m, n)
    (spx_trsm): side 'L' op(L) X = B with L (m, m), side 'R' X op(L) = B with
    L (n, n); ``trans`` selects op = transpose.  Asynchronous."""
    if side not in ('L', 'R'):
      raise ValueError("trsm: side must be 'L' or 'R', not %r" % (side,))
    m, n, ldb = self._matrix('trsm: B', B)
    dt = np_dtype(B.dtype)
    nl = m if side == 'L' else n
    _, _, ldl = self._matrix('trsm: L', L, nl, nl, dt)
    sd = 0 if side == 'L' else 1
    ws, nws = self._workspace_for('spx_trsm_workspace', (spx_dtype(dt), sd, m, n), B.device,
                                  'trsm: bad sizes (%d, %d)' % (m, n))
    if m == 0 or n == 0:
      return
    self._call('spx_trsm', spx_dtype(dt), sd, 1 if trans else 0, m, n, _ptr(L), ldl, _ptr(B), ldb, _ptr(ws), nws)

  def syrk(self, A, B, C, lower=False):
    """``C`` (M, N) -= ``A`` (M, K) @ ``B`` (N, K)^T (spx_syrk).  ``lower``
    (M == N): only C's lower triangle is read and written.  Asynchronous."""
    M, K, lda = self._matrix('syrk: A', A)
    dt = np_dtype(A.dtype)
    N, _, ldb = self._matrix('syrk: B', B, None, K, dt)
    _, _, ldc = self._matrix('syrk: C', C, M, N, dt)
    if lower and M != N:
      raise ValueError('syrk: lower needs a square C, got (%d, %d)' % (M, N))
    if M == 0 or N == 0 or K == 0:
      return
    self._call('spx_syrk', spx_dtype(dt), 1 if lower else 0, M, N, K, _ptr(A), lda, _ptr(B), ldb, _ptr(C), ldc)

  # ------------------------------------------------------------------- qr
  def geqr(self, A):
    """(R, handle) of the tall or square ``A`` (m, n), m >= n (spx_geqr): R is
    the new (n, n) upper-triangular factor with diag(R) >= 0 and +0.0 below the
    diagonal; ``handle`` owns the workspace with the reflectors for ``orgqr``.
    ``A`` is not written.  Asynchronous on the current stream."""
    import torch
    m, n, lda = self._matrix('geqr: A', A)
    dt = np_dtype(A.dtype)
    if m < n:
      raise ValueError('geqr: a tall or square matrix is needed, got %s' % ((m, n),))
    nmax, _ = geqr_plan(dt, n)
    if n > nmax:
      raise ValueError('geqr: %d columns are above the limit %d for %s' % (n, nmax, dt))
    need = self.lib.spx_geqr_workspace(spx_dtype(dt), m, n)
    if need < 0:
      raise ValueError('geqr: bad sizes (%d, %d)' % (m, n))
    R = torch.empty((n, n), dtype=A.dtype, device=A.device)
    ws = torch.empty((int(need),), dtype=torch.uint8, device=A.device)
    handle = QrHandle(ws, m, n, dt)
    if m == 0 or n == 0:
      return R, handle
    self._call('spx_geqr', spx_dtype(dt), m, n, _ptr(A), lda, _ptr(R), n, _ptr(ws), ws.numel())
    return R, handle

  def orgqr(self, handle, C, Q):
    """``Q`` (m, n) = Q_0 ``C`` for the factorization behind ``handle``: ``C``
    is the (n, n) seed, ``None`` for the identity (then A = Q R) (spx_orgqr).
    Asynchronous."""
    if not isinstance(handle, QrHandle):
      raise ValueError('orgqr: the handle of a geqr call is needed, got %r' % (type(handle).__name__,))
    m, n, dt = handle.m, handle.n, handle.dtype
    _, _, ldq = self._matrix('orgqr: Q', Q, m, n, dt)
    ldc = max(n, 1)
    if C is not None:
      _, _, ldc = self._matrix('orgqr: C', C, n, n, dt)
    if m == 0 or n == 0:
      return
    self._call('spx_orgqr', spx_dtype(dt), m, n, _ptr(handle.workspace), handle.workspace.numel(), _ptr(C), ldc,
               _ptr(Q), ldq)

  # ------------------------------------------------------------------ eigh
  def syevj(self, A, uplo='L'):
    """(W, V, info) of the symmetric ``A``, (n, n) or a batch (B, n, n)
    (spx_syevj): W (n,) / (B, n) the ascending eigenvalues, V of A's shape the
    eigenvectors as columns, ``info`` the int32 device tensor (one entry per
    matrix) of the sweeps used, -1 where a matrix did not converge or is not
    finite (its W and V are NaN); nothing here reads it.  Only the triangle
    ``uplo`` names is read; ``A`` needs unit stride on its last axis and a row
    stride of at least n, any batch stride, and is not written.  Asynchronous
    on the current stream."""
    import torch
    if uplo not in ('L', 'U'):
      raise ValueError("syevj: uplo must be 'L' or 'U', not %r" % (uplo,))
    if A.dim() not in (2, 3):
      raise ValueError('syevj: A must be 2-d or 3-d, got shape %s' % (tuple(A.shape),))
    dt = np_dtype(A.dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
      raise ValueError('syevj: A must be float32 / float64, not %s' % dt)
    n = int(A.shape[-1])
    if int(A.shape[-2]) != n:
      raise ValueError('syevj: square matrices are needed, got shape %s' % (tuple(A.shape),))
    nmax, _ = syevj_plan(dt)
    if n > nmax:
      raise ValueError('syevj: n = %d is above the limit %d for %s' % (n, nmax, dt))
    batch = int(A.shape[0]) if A.dim() == 3 else 1
    if batch > 0 and n > 1 and (A.stride(-1) != 1 or A.stride(-2) < n):
      raise ValueError('syevj: A needs unit stride on its last axis and a row stride of at least %d' % n)
    lda = int(A.stride(-2)) if n > 1 else max(n, 1)
    stride_a = int(A.stride(0)) if A.dim() == 3 and batch > 1 else 0
    W = torch.empty(tuple(A.shape[:-1]), dtype=A.dtype, device=A.device)
    V = torch.empty(tuple(A.shape), dtype=A.dtype, device=A.device)
    info = torch.zeros((batch,), dtype=torch.int32, device=A.device)
    if batch == 0 or n == 0:
      return W, V, info
    self._call('spx_syevj', spx_dtype(dt), 0 if uplo == 'L' else 1, batch, n, _ptr(A), lda, stride_a, _ptr(W), n,
               _ptr(V), n, n * n, _ptr(info))
    return W, V, info

  # ------------------------------------------------------------------- svd
  def gesvj(self, A, compute_uv=True):
    """(U, S, Vt, info) of ``A``, (m, n) or a batch (B, m, n) with m >= n
    (spx_gesvj): the reduced SVD A = U diag(S) Vt with S (n,) / (B, n)
    descending, U (.., m, n) and Vt (.., n, n); every row of Vt has its entry of
    largest magnitude positive, and the column of U of an exactly zero singular
    value is exactly zero.  With ``compute_uv`` false only S is computed and U
    and Vt are None.  ``info`` is the int32 device tensor (one entry per matrix)
    of the sweeps used, -1 where a matrix did not converge or is not finite
    (its outputs are NaN); nothing here reads it.  ``A`` needs unit stride on
    its last axis and a row stride of at least n, any batch stride, and is not
    written.  Asynchronous on the current stream."""
    import torch
    if A.dim() not in (2, 3):
      raise ValueError('gesvj: A must be 2-d or 3-d, got shape %s' % (tuple(A.shape),))
    dt = np_dtype(A.dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
      raise ValueError('gesvj: A must be float32 / float64, not %s' % dt)
    m, n = int(A.shape[-2]), int(A.shape[-1])
    if m < n:
      raise ValueError('gesvj: tall or square matrices are needed (m >= n), got shape %s' % (tuple(A.shape),))
    nmax, mmax, _ = gesvj_plan(dt, n)
    if n > nmax:
      raise ValueError('gesvj: n = %d is above the limit %d for %s' % (n, nmax, dt))
    if n > 0 and m > mmax:
      raise ValueError('gesvj: m = %d is above the limit %d for n = %d, %s' % (m, mmax, n, dt))
    batch = int(A.shape[0]) if A.dim() == 3 else 1
    if batch > 0 and n > 0 and ((n > 1 and A.stride(-1) != 1) or (m > 1 and A.stride(-2) < n)):
      raise ValueError('gesvj: A needs unit stride on its last axis and a row stride of at least %d' % n)
    lda = int(A.stride(-2)) if m > 1 else max(n, 1)
    stride_a = int(A.stride(0)) if A.dim() == 3 and batch > 1 else 0
    lead = tuple(A.shape[:-2])
    S = torch.empty(lead + (n,), dtype=A.dtype, device=A.device)
    U = Vt = None
    if compute_uv:
      U = torch.empty(lead + (m, n), dtype=A.dtype, device=A.device)
      Vt = torch.empty(lead + (n, n), dtype=A.dtype, device=A.device)
    info = torch.zeros((batch,), dtype=torch.int32, device=A.device)
    if batch == 0 or n == 0:
      return U, S, Vt, info
    self._call('spx_gesvj', spx_dtype(dt), 1 if compute_uv else 0, batch, m, n, _ptr(A), lda, stride_a, _ptr(U), n,
               m * n, _ptr(S), n, _ptr(Vt), n, n * n, _ptr(info))
    return U, S, Vt, info

  # ------------------------------------------------------- shortest paths
  def apsp(self, G, directed=True, unreachable=float('inf')):
    """(D, info): the all-pairs shortest path lengths of the edge-weight
    matrix ``G`` (n, n) (spx_apsp).  An off-diagonal entry is an edge iff it is
    finite and > 0 (0 and +inf: no edge; the diagonal is ignored); with
    ``directed`` false the edge between i and j is the smaller of those present
    in G[i, j] and G[j, i].  ``D`` is a new contiguous tensor of G's dtype with
    ``unreachable`` where there is no path; ``info`` the one-element int32
    device tensor, -1 when G holds a negative or NaN entry (D is then
    unspecified); nothing here reads it.  ``G`` needs unit stride on its last
    axis and a row stride of at least n, and is not written.  Asynchronous on
    the current stream."""
    import torch
    if G.dim() != 2:
      raise ValueError('apsp: G must be 2-d, got shape %s' % (tuple(G.shape),))
    dt = np_dtype(G.dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
      raise ValueError('apsp: G must be float32 / float64, not %s' % dt)
    n = int(G.shape[1])
    if int(G.shape[0]) != n:
      raise ValueError('apsp: a square matrix is needed, got shape %s' % (tuple(G.shape),))
    if n > 1 and (G.stride(1) != 1 or G.stride(0) < n):
      raise ValueError('apsp: G needs unit stride on its last axis and a row stride of at least %d' % n)
    unreachable = float(unreachable)
    if not unreachable >= 0.0:
      raise ValueError('apsp: unreachable = %r is negative or NaN' % unreachable)
    ldg = int(G.stride(0)) if n > 1 else max(n, 1)
    D = torch.empty((n, n), dtype=G.dtype, device=G.device)
    info = torch.zeros((1,), dtype=torch.int32, device=G.device)
    if n == 0:
      return D, info
    self._call('spx_apsp', spx_dtype(dt), 1 if directed else 0, n, _ptr(G), ldg, _ptr(D), n, unreachable, _ptr(info))
    return D, info

  # ---------------------------------------------------------- fuzzy k-means
  def fuzzy_step(self, points, centers, exponent, eps, weight_power, want_labels, want_U, sums=None, counts=None):
    """One fuzzy k-means step over ``points`` (N, D) float32 / float64 against
    ``centers`` (K, D) float64 (spx_fuzzy_step): with d_j = |x - c_j|^2 + eps,
    u_j = (dmin / d_j)^exponent / sum_j (dmin / d_j)^exponent per row.  Returns
    ``(labels, U, sums, counts)``: labels (N,) int64, the first index of the
    smallest d_j, with ``want_labels``, else None; U (N, K) in the points'
    dtype with ``want_U``, else None; sums (K, D) and counts (K,) float64 of
    u^weight_power x and u^weight_power.  Given ``sums`` and ``counts`` (both or
    neither), the step is ADDED to them; otherwise they are new tensors.
    ``points`` needs unit stride on its last axis and a row stride of at least
    D; any base address is served.  Asynchronous on the current stream."""
    import torch
    if points.dim() != 2:
      raise ValueError('fuzzy_step: points must be 2-d, got shape %s' % (tuple(points.shape),))
    dt = np_dtype(points.dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
      raise ValueError('fuzzy_step: points must be float32 / float64, not %s' % dt)
    N, D = int(points.shape[0]), int(points.shape[1])
    if centers.dim() != 2 or int(centers.shape[1]) != D or centers.dtype != torch.float64 or not centers.is_contiguous():
      raise ValueError('fuzzy_step: centers must be a contiguous float64 (K, %d) tensor' % D)
    K = int(centers.shape[0])
    if D < 1 or K < 1:
      raise ValueError('fuzzy_step: D = %d and K = %d must be at least 1' % (D, K))
    if N > 1 and (points.stride(1) != 1 or points.stride(0) < D) or N == 1 and D > 1 and points.stride(1) != 1:
      raise ValueError('fuzzy_step: points needs unit stride on its last axis and a row stride of at least %d' % D)
    for name, v in (('exponent', exponent), ('eps', eps), ('weight_power', weight_power)):
      if not (float(v) > 0.0 and np.isfinite(float(v))):
        raise ValueError('fuzzy_step: %s = %r is not finite and > 0' % (name, v))
    _rt, _g, kmax, need = fuzzy_plan(dt, N, D, K)
    if K > kmax:
      raise NotImplementedError('fuzzy_step: K = %d is above kmax = %d' % (K, kmax))
    if (sums is None) != (counts is None):
      raise ValueError('fuzzy_step: sums and counts are given together')
    add = sums is not None
    if add:
      _dense('fuzzy_step: sums', sums, np.dtype(np.float64), K * D, '%d x %d elements' % (K, D))
      _dense('fuzzy_step: counts', counts, np.dtype(np.float64), K, '%d elements' % K)
    else:
      sums = torch.empty((K, D), dtype=torch.float64, device=points.device)
      counts = torch.empty((K,), dtype=torch.float64, device=points.device)
    labels = torch.empty((N,), dtype=torch.int64, device=points.device) if want_labels else None
    U = torch.empty((N, K), dtype=points.dtype, device=points.device) if want_U else None
    key = (dt, D, K, points.device)
    ws = self._fuzzy_ws.get(key)
    if ws is None or ws.numel() < need:  # (kept per (dtype, D, K): its size does not depend on N)
      ws = self._fuzzy_ws[key] = torch.empty((max(need, 16),), dtype=torch.uint8, device=points.device)
    ldp = int(points.stride(0)) if N > 1 else D
    self._call('spx_fuzzy_step', spx_dtype(dt), N, D, K, _ptr(points), ldp, _ptr(centers), float(exponent),
               float(eps), float(weight_power), _ptr(labels), _ptr(U), K, _ptr(sums), _ptr(counts), 0 if add else 1,
               _ptr(ws), ws.numel())
    return labels, U, sums, counts

  # ------------------------------------------------------------------ n-body
  def nbody_accel(self, tx, ty, tz, sx, sy, sz, sm, G, rmin, splits=None):
    """``(ax, ay, az)``: the accelerations of the targets ``tx, ty, tz`` under
    the sources ``sx, sy, sz`` of mass ``sm`` (spx_nbody_accel): for target j,
    sum_i G sm_i (s_i - t_j) / r_i^3 with r_i = max(|s_i - t_j|, rmin).  All
    seven are contiguous 1-d tensors of one dtype (float32 / float64), the
    targets of one length and the sources of one length; the targets may be the
    sources.  The outputs are new tensors of the targets' length and dtype
    (zeros without sources).  ``splits``: None for the library's choice of
    source ranges, a positive number to force it.  Asynchronous on the current
    stream."""
    import torch
    _nbody_args('nbody_accel', (tx, ty, tz), (sx, sy, sz, sm), G, rmin)
    dt = np_dtype(tx.dtype)
    n_tgt, n_src = int(tx.numel()), int(sx.numel())
    splits = 0 if splits is None else int(splits)
    if splits < 0:
      raise ValueError('nbody_accel: splits = %d is negative' % splits)
    ax, ay, az = (torch.empty((n_tgt,), dtype=tx.dtype, device=tx.device) for _ in range(3))
    if n_tgt == 0:
      return ax, ay, az
    _tpb, use, need = nbody_plan(dt, n_tgt, n_src, splits)
    ws = self._nbody_ws.get(tx.device)
    if need and (ws is None or ws.numel() < need):  # (one per device, grown to the largest split seen)
      ws = self._nbody_ws[tx.device] = torch.empty((need,), dtype=torch.uint8, device=tx.device)
    self._call('spx_nbody_accel', spx_dtype(dt), n_tgt, _ptr(tx), _ptr(ty), _ptr(tz), n_src, _ptr(sx), _ptr(sy),
               _ptr(sz), _ptr(sm), float(G), float(rmin), _ptr(ax), _ptr(ay), _ptr(az), use,
               _ptr(ws if need else None), ws.numel() if need else 0)
    return ax, ay, az

  # ------------------------------------------------------- pairwise kernels
  def pairwise(self, X, Y, metric, gamma, out=None, row_sums=None, row_scale=None, col_scale=None, diag_col0=-1,
               diag_value=0.0, splits=None):
    """``(out, row_sums)`` of spx_pairwise: for the (n, d) rows of ``X`` and
    the (m, d) rows of ``Y`` (2-d tensors of one float32 / float64 dtype with
    unit column stride: column slices of wider tensors are accepted, and Y may
    be X) the values a_ij of ``metric`` ('sqeuclidean', 'euclidean',
    'manhattan', 'rbf' = exp(-gamma s_ij)), times ``row_scale[i] *
    col_scale[j]`` where the two (n,) / (m,) vectors are given.  ``out``: True
    for a new (n, m) tensor, a tensor (unit column stride) to fill, None / False
    for none; with ``diag_col0 >= 0`` its element (i, diag_col0 + i) is
    ``diag_value``.  ``row_sums``: True for a new (n,) tensor of sum_j of the
    computed values, a contiguous tensor to fill, None / False for none.  At
    least one of the two is wanted.  ``splits``: None for the library's choice
    of column ranges, a positive number to force it.  Asynchronous on the
    current stream."""
    import torch
    who = 'pairwise'
    for name, t in (('X', X), ('Y', Y)):
      if t.dim() != 2:
        raise ValueError('%s: %s must be 2-d, got shape %s' % (who, name, tuple(t.shape)))
    dt = np_dtype(X.dtype)
    if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
      raise ValueError('%s: X must be float32 / float64, not %s' % (who, dt))
    if np_dtype(Y.dtype) != dt:
      raise ValueError('%s: Y has dtype %s, X has %s: one dtype is needed' % (who, np_dtype(Y.dtype), dt))
    n, d = (int(v) for v in X.shape)
    m = int(Y.shape[0])
    if int(Y.shape[1]) != d:
      raise ValueError('%s: Y has %d features, X has %d' % (who, int(Y.shape[1]), d))
    if d < 1:
      raise ValueError('%s: X has no features (d = 0)' % who)
    if metric not in PAIR_METRICS:
      raise ValueError('%s: metric %r is not one of %s' % (who, metric, sorted(PAIR_METRICS)))
    gamma = float(gamma)
    if not (gamma >= 0.0 and np.isfinite(gamma)):
      raise ValueError('%s: gamma = %r is not finite and >= 0' % (who, gamma))
    splits = 0 if splits is None else int(splits)
    if splits < 0:
      raise ValueError('%s: splits = %d is negative' % (who, splits))

    def rows_of(name, t, rows, cols):  # the leading dimension of a 2-d operand with unit column stride
      if cols > 1 and t.stride(1) != 1:
        raise ValueError('%s: %s must have unit column stride, got strides %s' % (who, name, tuple(t.stride())))
      ld = int(t.stride(0)) if rows > 1 else cols
      if ld < cols:
        raise ValueError('%s: the rows of %s overlap (row stride %d, %d columns)' % (who, name, ld, cols))
      return ld

    ldx, ldy = rows_of('X', X, n, d), rows_of('Y', Y, m, d)
    if (row_scale is None) != (col_scale is None):
      raise ValueError('%s: row_scale and col_scale go together (both or neither)' % who)
    for name, t, size in (('row_scale', row_scale, n), ('col_scale', col_scale, m)):
      if t is not None:
        _dense('%s: %s' % (who, name), t, dt, size, '%d elements' % size)
    if out is None or out is False:
      out = None
    elif out is True:
      out = torch.empty((n, m), dtype=X.dtype, device=X.device)
    elif out.dim() != 2 or tuple(out.shape) != (n, m) or np_dtype(out.dtype) != dt:
      raise ValueError('%s: out must be a (%d, %d) %s tensor, got %s %s' % (who, n, m, dt, tuple(out.shape),
                                                                           np_dtype(out.dtype)))
    if row_sums is None or row_sums is False:
      row_sums = None
    elif row_sums is True:
      row_sums = torch.empty((n,), dtype=X.dtype, device=X.device)
    else:
      _dense('%s: row_sums' % who, row_sums, dt, n, '%d elements' % n)
    if out is None and row_sums is None:
      raise ValueError('%s: neither out nor row_sums is wanted' % who)
    ldo = rows_of('out', out, n, m) if out is not None else m
    diag_col0 = int(diag_col0)
    if diag_col0 < -1:
      raise ValueError('%s: diag_col0 = %d is below -1 (no diagonal)' % (who, diag_col0))
    if n == 0 or m == 0:
      if row_sums is not None:
        row_sums.zero_()
      return out, row_sums
    _tile, _kc, use, need = pairwise_plan(dt, n, m, splits)
    need = need if row_sums is not None else 0
    ws = self._pairwise_ws.get(X.device)
    if need and (ws is None or ws.numel() < need):  # (one per device, grown to the largest split seen)
      ws = self._pairwise_ws[X.device] = torch.empty((need,), dtype=torch.uint8, device=X.device)
    self._call('spx_pairwise', spx_dtype(dt), PAIR_METRICS[metric], n, m, d, _ptr(X), ldx, _ptr(Y), ldy, gamma,
               _ptr(out), ldo, _ptr(row_sums), _ptr(row_scale), _ptr(col_scale), diag_col0, float(diag_value), use,
               _ptr(ws if need else None), ws.numel() if need else 0)
    return out, row_sums

  # --------------------------------------------------------------- sparse
  @staticmethod
  def _csr(name, rowptr, col, val, n):
    """(m, nnz, dtype) of the CSR triple: rowptr (m + 1,) int64, col (nnz,)
    int32, val (nnz,) float32 / float64, all contiguous."""
    import torch
    if rowptr.dim() != 1 or rowptr.dtype != torch.int64 or rowptr.numel() < 1 or not rowptr.is_contiguous():
      raise ValueError('%s: rowptr must be a contiguous int64 vector of m + 1 entries' % name)
    if col.dim() != 1 or col.dtype != torch.int32 or not col.is_contiguous():
      raise ValueError('%s: col must be a contiguous int32 vector' % name)
    if val.dtype not in (torch.float32, torch.float64):
      raise ValueError('%s: val must be float32 / float64, not %s' % (name, val.dtype))
    dt = np_dtype(val.dtype)
    if val.dim() != 1 or val.numel() != col.numel() or not val.is_contiguous():
      raise ValueError('%s: val must be a contiguous vector of col\'s length' % name)
    if int(n) < 0 or int(n) > 2 ** 31 - 1:
      raise ValueError('%s: %d columns are outside the int32 range' % (name, n))
    return int(rowptr.numel()) - 1, int(col.numel()), dt

  def csrmm(self, rowptr, col, val, n, B, C, alpha=1.0, beta=0.0, g=0, workspace=None):
    """``C`` (m, p) = alpha A ``B`` + beta ``C`` for A (m, n) in CSR (spx_csrmm):
    ``B`` (n, p) and ``C`` may be padded (unit column stride); with beta == 0
    ``C`` is not read.  ``g`` fixes the lanes per row (0: the plan's).
    ``workspace`` is a ``CsrWorkspace`` that keeps the structure analysis of
    this matrix between calls (None: scratch of this call).  The columns must
    lie in [0, n): the kernel does not check them.  Asynchronous on the current
    stream; no host synchronisation."""
    import torch
    m, nnz, dt = self._csr('csrmm', rowptr, col, val, n)
    _, p, ldb = self._matrix('csrmm: B', B, int(n), None, dt)
    _, _, ldc = self._matrix('csrmm: C', C, m, p, dt)
    if m == 0 or p == 0:
      return
    if C.data_ptr() == B.data_ptr() and B.numel():
      raise ValueError('csrmm: C may not be B')
    need = int(self.lib.spx_csrmm_workspace(spx_dtype(dt), m, nnz, p))
    if need < 0:
      raise ValueError('csrmm: bad sizes (%d, %d, %d)' % (m, nnz, p))
    ws = workspace if workspace is not None else CsrWorkspace()
    if ws.buf is None or ws.buf.numel() < need or ws.buf.device != val.device:
      ws.buf, ws.prepared = torch.empty((need,), dtype=torch.uint8, device=val.device), False
    self._call('spx_csrmm', spx_dtype(dt), m, int(n), p, nnz, _ptr(rowptr), _ptr(col), _ptr(val), _ptr(B), ldb,
               _ptr(C), ldc, float(alpha), float(beta), int(g), _ptr(ws.buf), ws.buf.numel(), 1 if ws.prepared else 0)
    ws.prepared = True

  def csr_todense(self, rowptr, col, val, n, D):
    """``D`` (m, n), possibly padded, = the CSR matrix as a dense block
    (spx_csr_todense).  Asynchronous."""
    m, nnz, dt = self._csr('csr_todense', rowptr, col, val, n)
    _, _, ldd = self._matrix('csr_todense: D', D, m, int(n), dt)
    if m == 0 or n == 0:
      return
    self._call('spx_csr_todense', spx_dtype(dt), m, int(n), nnz, _ptr(rowptr), _ptr(col), _ptr(val), _ptr(D), ldd)

  def csr_rowids(self, rowptr, r0, out):
    """``out`` (nnz,) int32 = ``r0`` + the tile-local row of every stored entry
    of the CSR row pointers ``rowptr`` (spx_csr_rowids).  Asynchronous."""
    import torch
    if rowptr.dim() != 1 or rowptr.dtype != torch.int64 or rowptr.numel() < 1 or not rowptr.is_contiguous():
      raise ValueError('csr_rowids: rowptr must be a contiguous int64 vector of m + 1 entries')
    if out.dim() != 1 or out.dtype != torch.int32 or not out.is_contiguous():
      raise ValueError('csr_rowids: out must be a contiguous int32 vector')
    m, nnz = int(rowptr.numel()) - 1, int(out.numel())
    if int(r0) < 0 or int(r0) + m > 2 ** 31 - 1:
      raise ValueError('csr_rowids: rows %d .. %d are outside the int32 range' % (r0, int(r0) + m))
    if m == 0 or nnz == 0:
      return
    self._call('spx_csr_rowids', m, nnz, _ptr(rowptr), int(r0), _ptr(out))

  def als_solve(self, rowptr, col, val, n, Y, lam, X):
    """``X`` (m, f) = the ALS row solves of A (m, n) in CSR against the factor
    ``Y`` (n, f) with regularisation ``lam`` (spx_als_solve): row i solves
    (sum y y^T + lam |K_i| I) x = sum a y over the entries of the row whose
    value is not zero.  ``Y`` and ``X`` may be padded (unit column stride).
    Returns the one-element int32 device tensor ``info`` (the rows whose
    factorization failed, which hold NaN); nothing here reads it.  The columns
    must lie in [0, n).  Asynchronous on the current stream."""
    import torch
    m, nnz, dt = self._csr('als_solve', rowptr, col, val, n)
    _, f, ldy = self._matrix('als_solve: Y', Y, int(n), None, dt)
    _, _, ldx = self._matrix('als_solve: X', X, m, f, dt)
    fmax = als_plan(dt, 0)[0]
    if f < 1 or f > fmax:
      raise ValueError('als_solve: f = %d is outside [1, fmax = %d]' % (f, fmax))
    lam = float(lam)
    if not (lam >= 0.0 and np.isfinite(lam)):
      raise ValueError('als_solve: lam = %r is not finite and non-negative' % lam)
    if X.data_ptr() == Y.data_ptr() and Y.numel() and X.numel():
      raise ValueError('als_solve: X may not be Y')
    info = torch.zeros((1,), dtype=torch.int32, device=X.device)
    if m == 0:
      return info
    self._call('spx_als_solve', spx_dtype(dt), m, int(n), f, nnz, _ptr(rowptr), _ptr(col), _ptr(val), _ptr(Y), ldy,
               lam, _ptr(X), ldx, _ptr(info))
    return info

  @staticmethod
  def _kmeans_counters_offset(D):
    """Byte offset of KmWs::ctr (the 64-byte KmCounters block) in a
    spx_kmeans_assign / spx_kmeans_step workspace for K <= 256: it mirrors
    km_layout_assign in csrc/kmeans_kernels.h -- CT (D x 256 f32) | cn (256
    f64) | cmax (4 f64) | ctr.  The only Python statement of that layout."""
    return D * 256 * 4 + 256 * 8 + 32

  def kmeans_counters(self, D):
    """Diagnostic (tests, tools): KmCounters::n of the last spx_kmeans_assign
    / spx_kmeans_step workspace (K <= 256): [rows sent to the all-centre
    exact kernel, candidate rows, rows left undecided by the bf16x3 pass, rows
    left undecided by the fp16 screen]."""
    import torch
    off = self._kmeans_counters_offset(D)
    return self._ws[off:off + 16].view(torch.int32).cpu().tolist()

  def kmeans_candidates(self, D, N, count):
    """Diagnostic (tools): the first ``count`` entries of KmWs::cand_list of
    that workspace as raw bytes, (count, 40) uint8 -- KfCand = {i64 row; u32
    mask[8]}.  The list follows KmCounters (64 bytes) and the full list (N i64)."""
    base = self._kmeans_counters_offset(D) + 64 + N * 8
    return self._ws[base:base + count * 40].cpu().numpy().reshape(-1, 40)

  def _workspace(self, nbytes, device):
    """Grow-only scratch buffer on ``device`` (reuse is stream-ordered)."""
    import torch
    ws = getattr(self, '_ws', None)
    if ws is None or ws.numel() < nbytes or ws.device != device:
      ws = torch.empty((nbytes,), dtype=torch.uint8, device=device)
      self._ws = ws
    return ws

  @staticmethod
  def _f64():
    import torch
    return torch.float64


def out_device(inputs, slots):
  import torch
  if slots:
    return inputs[slots[0]].device
  return torch.device('cuda', torch.cuda.current_device())


def _cls(stride):
  return 'c' if stride == 1 else ('b' if stride == 0 else 'g')


def _dense(what, t, dtype, numel, size):
  """ValueError unless ``t`` is a contiguous ``dtype`` tensor of ``numel``
  elements (``size``: how the message words that count)."""
  if np_dtype(t.dtype) != dtype or not t.is_contiguous() or t.numel() != numel:
    raise ValueError('%s must be a contiguous %s tensor of %s' % (what, dtype, size))


def _nbody_args(who, targets, sources, G, rmin):
  """ValueError unless the n-body operands are contiguous 1-d tensors of one
  float32 / float64 dtype, of one length within each group, with a finite G
  and a finite rmin >= 0."""
  dt = np_dtype(targets[0].dtype)
  if dt not in (np.dtype(np.float32), np.dtype(np.float64)):
    raise ValueError('%s: the arrays must be float32 / float64, not %s' % (who, dt))
  for name, group in (('targets', targets), ('sources', sources)):
    for t in group:
      if t.dim() != 1 or not t.is_contiguous():
        raise ValueError('%s: the %s must be contiguous 1-d tensors, got shape %s' % (who, name, tuple(t.shape)))
      if np_dtype(t.dtype) != dt:
        raise ValueError('%s: one dtype is needed, got %s and %s' % (who, dt, np_dtype(t.dtype)))
      if t.numel() != group[0].numel():
        raise ValueError('%s: the %s have unequal lengths %d and %d' % (who, name, group[0].numel(), t.numel()))
  if not np.isfinite(float(G)):
    raise ValueError('%s: G = %r is not finite' % (who, G))
  if not (float(rmin) >= 0.0 and np.isfinite(float(rmin))):
    raise ValueError('%s: rmin = %r is not finite and >= 0' % (who, rmin))


def _vec_aligned(t, strides, cls, V):
  if cls == 'c':
    return t.data_ptr() % (V * t.element_size()) == 0 and all(s % V == 0 for s in strides[:-1])
  return True


def _scalars_into(root, args):
  for node in codegen.walk(root):
    if isinstance(node, codegen.Sc):
      if node.pytype is float:
        args.fsc[node.slot] = node.value
      else:
        args.isc[node.slot] = int(node.value)


# ----------------------------------------------------------- active backend
_backend = None


def get():
  global _backend
  if _backend is None:
    _backend = HipBackend()
  return _backend


def set_backend(b):
  """Install a backend object (tests only); returns the previous one."""
  global _backend
  prev = _backend
  _backend = b
  return prev
