"""The C-ABI library loads and exports every entry point include/spx.h declares
(no compute calls: those need a GPU)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'spartan_amd', 'libspx.so')


def declared():
  src = open(os.path.join(ROOT, 'include', 'spx.h')).read()
  return sorted(set(re.findall(r'\b(spx_[a-z_]+)\s*\(', src)))


def test_header_lists_the_boundary():
  names = declared()
  for n in ['spx_abi_version', 'spx_last_error', 'spx_module_load', 'spx_module_function', 'spx_launch',
            'spx_fill', 'spx_reduce_finalize', 'spx_merge', 'spx_copy_region', 'spx_gemm', 'spx_gemm_plan',
            'spx_argreduce_combine', 'spx_module_unload', 'spx_comm_load', 'spx_comm_unique_id',
            'spx_comm_init', 'spx_comm_destroy', 'spx_allreduce', 'spx_reduce_scatter', 'spx_allgather',
            'spx_broadcast', 'spx_reduce', 'spx_sendrecv']:
    assert n in names


@pytest.mark.skipif(not os.path.exists(LIB), reason='libspx.so not built')
def test_library_exports_every_declared_symbol():
  import torch  # noqa: F401  (torch's HIP runtime first)
  lib = ctypes.CDLL(LIB)
  for n in declared():
    assert hasattr(lib, n), n
  lib.spx_abi_version.restype = ctypes.c_int
  assert lib.spx_abi_version() == 3


@pytest.mark.skipif(not os.path.exists(LIB), reason='libspx.so not built')
def test_python_binding_signatures_cover_header():
  from spartan_amd import backend
  assert sorted(backend.EXPORTED) == declared()


C_CLASS = {'int': 'i4', 'int32_t': 'i4', 'uint32_t': 'i4', 'int64_t': 'i8', 'uint64_t': 'i8', 'size_t': 'i8',
           'double': 'f8'}


def prototypes():
  """{name: (return class, [argument classes])} of every prototype in
  include/spx.h: 'p' for a pointer, else the kind and the bytes of the type."""
  src = open(os.path.join(ROOT, 'include', 'spx.h')).read()
  src = re.sub(r'/\*.*?\*/', ' ', src, flags=re.S)
  src = re.sub(r'//[^\n]*', ' ', src)
  src = '\n'.join(line for line in src.split('\n') if not line.lstrip().startswith('#'))

  def cls(decl, named):
    if '*' in decl or '[' in decl:
      return 'p'
    words = [w for w in decl.split() if w not in ('const', 'unsigned', 'signed')]
    assert len(words) == (2 if named else 1), decl
    return C_CLASS[words[0]]

  out = {}
  for ret, name, args in re.findall(r'([A-Za-z_][\w\s\*]*?)\b(spx_\w+)\s*\(([^()]*)\)\s*;', src):
    args = [a.strip() for a in args.split(',')] if args.strip() not in ('', 'void') else []
    assert name not in out, name
    out[name] = (cls(ret, False), [cls(a, True) for a in args])
  return out


def ctypes_class(t):
  if t in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(t, ctypes._Pointer):
    return 'p'
  return ('f' if t in (ctypes.c_float, ctypes.c_double) else 'i') + str(ctypes.sizeof(t))


def test_python_binding_signatures_match_header_prototypes():
  """Every prototype of include/spx.h has an entry in the binding's ctypes
  table with the same arity and, per argument and for the result, the same
  class: pointer, or integer / float of the same width.  A wrong width or a
  missing argument there would corrupt a call silently.  (Needs neither the
  built library nor a GPU.)"""
  from spartan_amd import binding
  protos = prototypes()
  assert sorted(protos) == declared() and len(protos) >= 68
  for name, (ret, args) in protos.items():
    assert name in binding._SIGS, name
    argtypes, restype = binding._SIGS[name]
    assert len(argtypes) == len(args), (name, len(argtypes), len(args))
    assert [ctypes_class(t) for t in argtypes] == args, name
    assert ctypes_class(restype) == ret, name
  # and the parser tells the classes apart
  assert protos['spx_last_error'] == ('p', []) and protos['spx_kmeans_assign_workspace'] == ('i8', ['i4'] + ['i8'] * 3)
  assert protos['spx_gemm'][1][-3:] == ['f8', 'f8', 'p'] and protos['spx_launch'][1][1] == 'i4'
  assert protos['spx_gemm_plan'] == ('i4', ['i4', 'i8', 'i8', 'i8', 'p', 'i8', 'p', 'i8'] + ['p'] * 6)


def test_binding_module_stands_alone():
  """spartan_amd/binding.py imports nothing else of the package: loaded by its
  path in a fresh interpreter it brings in neither the backend nor codegen,
  and the table and the dtype codes are there without a GPU."""
  import subprocess
  import sys
  code = r'''
import importlib.util, sys
spec = importlib.util.spec_from_file_location('binding', %r)
m = importlib.util.module_from_spec(spec)
spec.loader.exec_module(m)
assert len(m.EXPORTED) >= 68 and m.spx_dtype('float32') == m.SPX_F32
assert not [k for k in sys.modules if k.startswith('spartan_amd') or k == 'torch'], sorted(sys.modules)
print('ok')
''' % os.path.join(ROOT, 'spartan_amd', 'binding.py')
  r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=120)
  assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stderr[-2000:]


@pytest.mark.skipif(not os.path.exists(LIB), reason='libspx.so not built')
def test_argument_validation_without_gpu():
  """Invalid arguments are rejected before any device work (error codes + message)."""
  import torch  # noqa: F401
  lib = ctypes.CDLL(LIB)
  lib.spx_last_error.restype = ctypes.c_char_p
  I64 = ctypes.c_int64 * 1
  rc = lib.spx_fill(ctypes.c_int(99), ctypes.c_int(0), None, ctypes.c_int(1), I64(4), I64(0), I64(4),
                    ctypes.c_double(0), ctypes.c_double(0), ctypes.c_uint64(0), None)
  assert rc == -1 and b'dtype' in lib.spx_last_error()
  rc = lib.spx_gemm(ctypes.c_int(0), ctypes.c_int64(4), ctypes.c_int64(4), ctypes.c_int64(4), None,
                    ctypes.c_int64(4), None, ctypes.c_int64(4), None, ctypes.c_int64(4),
                    ctypes.c_double(1), ctypes.c_double(0), None)
  assert rc == -3 and b'not supported' in lib.spx_last_error()
  rc = lib.spx_gemm(ctypes.c_int(3), ctypes.c_int64(4), ctypes.c_int64(4), ctypes.c_int64(8), None,
                    ctypes.c_int64(4), None, ctypes.c_int64(4), None, ctypes.c_int64(4),
                    ctypes.c_double(1), ctypes.c_double(0), None)
  assert rc == -1 and b'leading dimension' in lib.spx_last_error()


def _gemm_plans(p3_env, cases):
  """binding.gemm_plan of every (dtype, M, N, K, a_ptr, lda, b_ptr, ldb) of
  ``cases`` in a fresh interpreter with SPX_GEMM_P3 = ``p3_env`` (None: not
  set) -- the library reads the switch once per process."""
  import json
  import subprocess
  import sys
  code = r'''
import json, sys
sys.path.insert(0, %r)
from spartan_amd import binding
print(json.dumps([binding.gemm_plan(*c) for c in json.loads(sys.argv[1])]))
''' % ROOT
  env = {k: v for k, v in os.environ.items() if k != 'SPX_GEMM_P3'}
  if p3_env is not None:
    env['SPX_GEMM_P3'] = str(p3_env)
  r = subprocess.run([sys.executable, '-c', code, json.dumps(cases)], capture_output=True, text=True, timeout=120,
                     env=env)
  assert r.returncode == 0, r.stderr[-2000:]
  return json.loads(r.stdout.strip().split('\n')[-1])


@pytest.mark.skipif(not os.path.exists(LIB), reason='libspx.so not built')
def test_gemm_route_table_without_gpu():
  """spx_gemm_plan at the boundaries of spx_gemm's selection, with made-up
  operand addresses (never dereferenced): the 512-big-tile and 1024-fp64-tile
  thresholds, the alignment predicates one at a time, the SPX_GEMM_P3 switch,
  the integer dtypes and the argument errors of spx_gemm."""
  P = 0x10000  # a 16-byte aligned address

  def case(dt, M, N, K, a=P, lda=None, b=P, ldb=None):
    return [dt, M, N, K, a, K if lda is None else lda, b, N if ldb is None else ldb]

  f32 = [
    (case('float32', 1792, 18688, 16), 'F32_SMALL', True),    # 7 x 73 = 511 big tiles
    (case('float32', 1792, 18689, 16), 'F32_BIG', False),     # 7 x 74 = 518
    (case('float32', 4096, 8192, 16), 'F32_P3', True),        # 16 x 32 = 512, whole 256 x 256 tiles
    (case('float32', 4093, 8187, 19), 'F32_BIG', False),      # 512, edge tiles
    (case('float32', 3841, 8192, 16), 'F32_BIG', False),      # 512 with one row in the last tile row
    (case('float32', 3840, 8192, 16), 'F32_SMALL', True),     # 15 x 32 = 480
    (case('float32', 4096, 8320, 16), 'F32_BIG', True),       # N % 256 == 128: whole 256 x 128 tiles only
    (case('float32', 4096, 8320, 8208), 'F32_BIG', True),
    (case('float32', 1, 130817, 33), 'F32_BIG', False),       # 1 x 512
    (case('float32', 1, 130816, 33), 'F32_SMALL', False),     # 1 x 511
    (case('float32', 128, 128, 16), 'F32_SMALL', True),
    (case('float32', 1, 1, 1), 'F32_SMALL', False),
  ]
  # each alignment predicate alone turns `aligned` off (and P3 into BIG)
  for M, N, kern in [(128, 128, 'F32_SMALL'), (4096, 8320, 'F32_BIG'), (4096, 8192, 'F32_BIG')]:
    f32 += [
      (case('float32', M, N, 16, a=P + 4), kern, False),
      (case('float32', M, N, 16, b=P + 4), kern, False),
      (case('float32', M, N, 16, lda=17), kern, False),
      (case('float32', M, N, 16, ldb=N + 2), kern, False),
      (case('float32', M, N, 17), kern, False),
      (case('float32', M, N, 15), kern, False),
      (case('float32', M, N, 16, lda=20, ldb=N + 4), 'F32_P3' if N == 8192 else kern, True),  # padded rows stay aligned
    ]
  f64 = [
    (case('float64', 3968, 4224, 16), 'F64', True),           # 31 x 33 = 1023 tiles
    (case('float64', 4096, 4096, 16), 'F64', True),           # 1024: F64_P3 only with SPX_GEMM_P3=2
    (case('float64', 4096, 4096, 8208), 'F64', True),
    (case('float64', 4093, 4091, 19), 'F64', False),
    (case('float64', 128, 128, 16), 'F64', True),
    (case('float64', 128, 128, 16, a=P + 8), 'F64', False),
    (case('float64', 128, 128, 16, b=P + 8), 'F64', False),
    (case('float64', 128, 128, 16, lda=17), 'F64', False),
    (case('float64', 128, 128, 16, ldb=129), 'F64', False),
    (case('float64', 128, 128, 16, lda=18, ldb=130), 'F64', True),
    (case('float64', 128, 128, 17), 'F64', False),
    (case('float64', 127, 128, 16), 'F64', False),
    (case('float64', 128, 129, 16), 'F64', False),
  ]
  ints = [(case(dt, M, N, K), 'INT', False)
          for dt in ('int32', 'int64') for M, N, K in [(1, 1, 1), (16, 16, 16), (4096, 8192, 16), (33, 50, 100)]]
  table = f32 + f64 + ints
  got = _gemm_plans(None, [c for c, _, _ in table])
  tile = {'INT': (16, 16, 16, 0), 'F32_SMALL': (128, 128, 16, 8192), 'F32_BIG': (256, 128, 16, 8192),
          'F32_P3': (256, 256, 16, 8192), 'F64': (128, 128, 16, 0), 'F64_P3': (128, 128, 16, 8192)}
  for (c, kern, aligned), g in zip(table, got):
    assert (g['kernel'], g['aligned']) == (kern, aligned), (c, g)
    assert (g['bm'], g['bn'], g['bk'], g['flush_k']) == tile[kern], (c, g)

  # SPX_GEMM_P3=2: fp64 goes to the three-stage kernel at >= 1024 whole tiles only; fp32 as by default
  on2 = [(case('float64', 4096, 4096, 16), 'F64_P3', True), (case('float64', 4096, 4096, 8208), 'F64_P3', True),
         (case('float64', 3968, 4224, 16), 'F64', True), (case('float64', 4093, 4091, 19), 'F64', False),
         (case('float64', 4096, 4096, 16, a=P + 8), 'F64', False), (case('float64', 4096, 4096, 18), 'F64', False),
         (case('float32', 4096, 8192, 16), 'F32_P3', True)]
  # SPX_GEMM_P3=0: the two-stage kernels everywhere
  off = [(case('float32', 4096, 8192, 16), 'F32_BIG', True), (case('float32', 1792, 18688, 16), 'F32_SMALL', True),
         (case('float64', 4096, 4096, 16), 'F64', True)]
  for env, tab in ((2, on2), (0, off)):
    for (c, kern, aligned), g in zip(tab, _gemm_plans(env, [c for c, _, _ in tab])):
      assert (g['kernel'], g['aligned']) == (kern, aligned), (env, c, g)
      assert (g['bm'], g['bn'], g['bk'], g['flush_k']) == tile[kern], (env, c, g)

  # the argument errors, in spx_gemm's order, and nothing written on an error
  from spartan_amd import binding
  lib = binding.load_library()
  out = [ctypes.c_int64(-7) for _ in range(6)]

  def rc(dt, M, N, K, a=P, lda=None, b=P, ldb=None):
    return lib.spx_gemm_plan(dt, M, N, K, ctypes.c_void_p(a), K if lda is None else lda, ctypes.c_void_p(b),
                             N if ldb is None else ldb, *[ctypes.byref(x) for x in out])

  F32, F64, I32, BOOL = binding.SPX_F32, binding.SPX_F64, binding.SPX_I32, binding.SPX_BOOL
  for bad, want, word in [((BOOL, 4, 4, 4), -3, b'not supported'), ((9, 4, 4, 4), -3, b'not supported'),
                          ((F32, -1, 4, 4), -1, b'negative'), ((F32, 4, 4, -1), -1, b'negative'),
                          ((F32, 4, 4, 8, P, 7), -1, b'leading dimension'),
                          ((F64, 4, 8, 4, P, 4, P, 7), -1, b'leading dimension'),
                          ((F32, 4, 4, 4, 0), -1, b'null'), ((I32, 4, 4, 4, P, 4, 0), -1, b'null'),
                          ((F32, 4, 4, 0), -3, b'K == 0'), ((I32, 4, 4, 0), -3, b'K == 0'),
                          ((F32, 256 << 16, 256 << 16, 16), -1, b'too many tiles'),
                          ((F64, 128 << 16, 128 << 16, 16), -1, b'too many tiles')]:
    assert rc(*bad) == want and word in lib.spx_last_error(), (bad, lib.spx_last_error())
    assert [x.value for x in out] == [-7] * 6, bad
  # an empty product is no error and launches nothing, whatever the pointers and K
  for empty in [(F32, 0, 4, 4), (F64, 4, 0, 4), (I32, 0, 0, 0), (F32, 0, 4, 0, 0, 0, 0)]:
    assert rc(*empty) == 0 and out[0].value == 0 and binding.GEMM_KERNELS[0] == 'NONE', empty
  # every output is optional
  assert lib.spx_gemm_plan(F32, 4, 4, 4, ctypes.c_void_p(P), 4, ctypes.c_void_p(P), 4, *[None] * 6) == 0
  with pytest.raises(ValueError, match='leading dimension'):
    binding.gemm_plan('float32', 4, 4, 8, lda=4)


@pytest.mark.skipif(not os.path.exists(LIB), reason='libspx.so not built')
def test_collectives_boundary_without_gpu():
  """RCCL is opened at run time: before spx_comm_load every collective
  refuses; after it (PyTorch's own RCCL) a unique id can be made without a
  device; bad dtypes / ops are rejected before RCCL sees them."""
  import subprocess
  import sys
  code = r'''
import ctypes, sys
sys.path.insert(0, %r)
from spartan_amd import backend, comm
lib = backend.load_library()
assert lib.spx_allreduce(None, None, None, 4, 3, 0, None) == -1
assert b'spx_comm_load' in lib.spx_last_error()
uid = comm.rccl_unique_id()
assert len(uid) == 128 and any(uid)
assert lib.spx_allreduce(ctypes.c_void_p(1), None, None, 4, 9, 0, None) == -1
assert b'dtype' in lib.spx_last_error()
assert lib.spx_reduce_scatter(ctypes.c_void_p(1), None, None, 4, 3, 4, None) == -1
assert b'op' in lib.spx_last_error()
assert lib.spx_comm_init(uid, 128, 2, 2, ctypes.byref(ctypes.c_void_p())) == -1
assert lib.spx_comm_load(b'/nonexistent/librccl.so') == 0  # already loaded: a no-op
print('ok')
''' % ROOT
  r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=120)
  assert r.returncode == 0 and r.stdout.strip().endswith('ok'), r.stderr[-2000:]


# (dtype, N, D, K, assign, accumulate, step): the three workspace sizes as the
# hand-written formulas before the single layout routines returned them
# (recorded from a build of that commit; CU count 256, the no-device default
# and the MI355X's)
KM_WORKSPACE = [
  ('F32', 0, 64, 8, 67936, 4160, 206500),
  ('F32', 1, 3, 1, 5300, 32, 7316),
  ('F32', 31, 64, 256, 69928, 133120, 4466288),
  ('F32', 4097, 128, 256, 396968, 34080768, 60074624),
  ('F32', 70001, 128, 100, 4631296, 26419200, 48235216),
  ('F32', 9000, 130, 300, 342432, 20121600, 71075916),
  ('F32', 100000000, 128, 256, 6425133728, 67633152, 8190590372),
  ('F64', 31, 64, 256, 69928, 266240, 4599408),
  ('F64', 4097, 128, 256, 396968, 67633152, 93627008),
  ('F32', 4097, 64, 33, 331176, 2213640, 4245384),
  ('F32', 32, 64, 1, 69992, 520, 88704),
  ('F32', 33, 128, 32, 135856, 66048, 1285008),
  ('F32', 8192, 64, 64, 594272, 8519680, 14558568),
  ('F32', 8193, 64, 65, 594344, 8652800, 14775684),
  ('F32', 262144, 64, 128, 16910688, 17039360, 46927332),
  ('F32', 262145, 128, 129, 16976552, 34080768, 74686208),
  ('F32', 1000003, 64, 257, 8135288, 17105920, 55322520),
  ('F32', 5, 1, 1, 3500, 16, 5036),
  ('F32', 12345, 7, 513, 126504, 2790720, 8670548),
  ('F64', 0, 1, 1, 3172, 16, 4720),
  ('F64', 70001, 128, 100, 4631296, 26419200, 48235216),
  ('F64', 9000, 130, 300, 342432, 20121600, 71075916),
  ('F32', 2000000, 128, 256, 128633728, 67633152, 255736184),
  ('F32', 8191, 17, 256, 545892, 9437184, 16148576),
]


@pytest.mark.skipif(not os.path.exists(LIB), reason='libspx.so not built')
def test_kmeans_workspace_sizes_without_gpu():
  """The k-means workspace sizes come from a counting run of the layout
  routines that also carve the workspace; the memory footprint stays where
  the earlier formulas had it: within 1 KiB (four 256-byte alignment slacks)
  either way.  Bad arguments still return -1."""
  import torch  # noqa: F401
  lib = ctypes.CDLL(LIB)
  fns = [getattr(lib, 'spx_kmeans_%s_workspace' % n) for n in ('assign', 'accumulate', 'step')]
  for f in fns:
    f.restype = ctypes.c_int64
    f.argtypes = [ctypes.c_int] + [ctypes.c_int64] * 3
  code = {'F32': 3, 'F64': 4}
  for dt, N, D, K, *want in KM_WORKSPACE:
    for f, parent in zip(fns, want):
      new = f(code[dt], N, D, K)
      assert parent - 1024 <= new <= parent + 1024, (f.__name__, dt, N, D, K, new, parent)
  for bad in [(3, 1, 0, 1), (3, 1, 1, 0), (3, -1, 1, 1), (2, 1, 1, 1), (5, 1, 1, 1), (0, 1, 1, 1)]:
    for f in fns:
      assert f(*bad) == -1, (f.__name__, bad)
