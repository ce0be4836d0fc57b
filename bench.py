#!/usr/bin/env python3
"""Headline benchmark: fused map+reduce GB/s (+ dot GFLOP/s) on MI355X.

Workload (BASELINE.json configs[1]): x, y ~ U[0,1), z ~ U[-1,1) fp32, 2^30
elements (32768 x 32768) per GPU, resident in HBM before timing; one step =
``sum(x*y + exp(z), axis=0).optimized().force()`` and the same for axis=1 --
two fused map+reduce evaluations, each reading 3 x 4 B per element and writing
32768 fp32 per GPU.  ``value`` = algorithmic bytes of all ranks / the max over
ranks of the timed wall time.  Multi-GPU: launched by torchrun, one rank per
GPU; the global arrays are (32768 * N, 32768), row-strip tiled so every rank
owns one 2^30-element strip (weak scaling: per-GPU work fixed); the axis-0 sum
combines the per-rank partials with an RCCL reduce-scatter, the axis-1 sum is
local.  ``--strong`` keeps the global array at 2^30 instead.

A plain run sets up, warms up, times ``--steps`` steps and prints the result
line; ``--dump-outputs DIR`` also writes the last timed step's two results.
``--full`` adds everything else: the cold-start probe, the post-timing checks
against fp64 restatements, the axis=None / materialised-map extras, the vendor
reduction, ``dot(A, B)`` for 32768^2 fp32 / fp64 (configs[3]) in GFLOP/s, the
lreg and k-means legs, and the CPU baseline (the reference's multi-worker NumPy
model, oracle/cpu_baseline.py) on a bounded sample; ``--dot``, ``--workloads``
and ``--cpu-baseline`` choose among those legs.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: 8.0 TB/s spec
MFMA_F32_TFS = 157.3       # dense fp32 MFMA (v_mfma_f32_32x32x2_f32)
MFMA_F64_TFS = 78.6        # dense fp64 MFMA


def launch_ranks(n, argv):
  """``--gpus N`` without a torchrun environment: start N ranks with
  torch.distributed.run as a CHILD process (never exec: this process has not
  touched the GPU and must not be replaced), relay rank 0's JSON line and
  exit with the child's status (non-zero if any rank failed).  Reference
  harness: tests/test_common.py:102-121 sweeps its worker counts itself."""
  import socket
  import subprocess
  s = socket.socket()
  s.bind(('127.0.0.1', 0))
  port = s.getsockname()[1]
  s.close()
  cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(n),
         '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)] + argv
  env = dict(os.environ)
  env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
  proc = subprocess.Popen(cmd, stdout=subprocess.PIPE, env=env, text=True)
  line = None
  for raw in proc.stdout:  # stream: progress lines pass through as they come
    if raw.startswith('{') and '"metric"' in raw:
      line = raw.strip()
    else:
      sys.stdout.write(raw)
      sys.stdout.flush()
  rc = proc.wait()
  if line is not None:
    print(line, flush=True)
  if rc != 0 or line is None:
    sys.stderr.write('bench.py: %d-rank run failed (exit %d%s)\n' % (n, rc, '' if line else ', no result line'))
    return rc or 1
  return 0


def main():
  if '--gpus' in sys.argv or any(a.startswith('--gpus=') for a in sys.argv):
    pre = argparse.ArgumentParser(add_help=False)
    pre.add_argument('--gpus', type=int, default=1)
    known, _ = pre.parse_known_args()
    if known.gpus > 1 and 'WORLD_SIZE' not in os.environ:
      sys.exit(launch_ranks(known.gpus, sys.argv[1:]))
  ap = argparse.ArgumentParser()
  ap.add_argument('--gpus', type=int, default=1)
  ap.add_argument('--steps', type=int, default=10)
  ap.add_argument('--warmup', type=int, default=2)
  ap.add_argument('--size', type=int, default=32768)
  ap.add_argument('--full', action='store_true',
                  help='also run the cold-start probe, the post-timing checks, the cfg2 extras, the vendor '
                       'comparisons, the dot / lreg / k-means legs and the CPU baseline (off: the headline only)')
  ap.add_argument('--dump-outputs', metavar='DIR', default=None,
                  help='write the results of the last timed step to DIR/axis0.npy and DIR/axis1.npy (float32)')
  ap.add_argument('--dot', type=int, default=1, help='--full: also time the dot config (1/0)')
  ap.add_argument('--dot-size', type=int, default=32768)
  ap.add_argument('--cpu-baseline', type=int, default=1, help='--full: also run the CPU baseline (1/0)')
  ap.add_argument('--cpu-rows', type=int, default=32768, help='rows of the CPU baseline sample (full cfg2 strip: ~10-20 s of CPU work)')
  ap.add_argument('--strong', action='store_true', help='fixed 2^30 global array (strong scaling)')
  ap.add_argument('--workloads', default='1',
                  help='--full: also time k-means (cfg3) and lreg (cfg5): 1 / 0, or a comma list of lreg, kmeans, '
                       'kmeans_api')
  ap.add_argument('--km-points', type=int, default=100000000)
  ap.add_argument('--lreg-points', type=int, default=100000000)
  args = ap.parse_args()
  if args.steps < 1 or args.warmup < 0:
    ap.error('--steps must be at least 1 and --warmup at least 0')

  import torch
  import spartan_amd
  from spartan_amd import backend, comm, expr, runtime

  try:
    ctx = spartan_amd.initialize()
  except runtime.DataPlaneError as e:
    # the data plane's start-up self-test names the failing collective
    sys.stderr.write('bench.py: rank %s: %s\n' % (os.environ.get('RANK', '0'), e))
    sys.exit(4)
  be = backend.get()
  assert isinstance(be, backend.HipBackend)
  S = args.size
  N = ctx.world_size
  if N != args.gpus:
    raise SystemExit('bench.py: --gpus %d but the launcher started %d ranks' % (args.gpus, N))

  def sync():
    torch.cuda.synchronize()

  R = S if args.strong else S * N   # global rows
  x = expr.rand(R, S, dtype=np.float32, seed=11).force()
  y = expr.rand(R, S, dtype=np.float32, seed=12).force()
  z = expr.rand(R, S, dtype=np.float32, seed=13, low=-1.0, high=1.0).force()
  X, Y, Z = expr.lazify(x), expr.lazify(y), expr.lazify(z)

  def step():
    a0 = expr.sum(X * Y + expr.exp(Z), axis=0).optimized().force()
    a1 = expr.sum(X * Y + expr.exp(Z), axis=1).optimized().force()
    return a0, a1

  cold = cold_start(expr, X, Y, Z, sync) if args.full else None
  for _ in range(args.warmup):
    step()
  sync()
  comm.barrier()
  sync()
  be.kernel_events = []
  t0 = time.perf_counter()
  for _ in range(args.steps):
    last = step()
  sync()
  comm.barrier()
  sync()
  elapsed = time.perf_counter() - t0
  events = be.kernel_events
  be.kernel_events = None
  elapsed = comm.max_over_ranks(elapsed)

  elems = R * S
  bytes_per_eval = 3 * 4 * elems + 4 * S * N   # + each rank's output write
  total_bytes = 2 * bytes_per_eval * args.steps
  value = total_bytes / elapsed / 1e9
  # dominant kernel: the generated fused map+reduce kernel ('spx_reduce'),
  # timed with HIP events on the stream it is launched on
  red = [(s.elapsed_time(e) * 1e-3) for (n, s, e) in events if n.startswith('spx_reduce')]
  knames = sorted({n for (n, s, e) in events if n.startswith('spx_reduce')})
  ax0 = red[0::2]
  ax1 = red[1::2]
  rows_local = sum(ex.shape[0] for ex in x.local) if hasattr(x, 'local') else S
  bytes_launch = 3 * 4 * rows_local * S + 4 * S
  avg = float(np.mean(red)) if red else float('nan')
  achieved = bytes_launch / avg / 1e9 if red else None

  traffic = None
  tname = 'r05_cfg2_pmc_traffic.json'
  tpath = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'profiles', tname)
  if os.path.exists(tpath) and rows_local == 32768 and S == 32768:
    with open(tpath) as f:
      traffic = json.load(f)['hbm_bytes_per_launch']
  result = {
      'metric': 'fused map+reduce GB/s (x*y+exp(z), sum axis 0 and axis 1, 2^30 fp32 per GPU)',
      'value': round(value, 2),
      'unit': 'GB/s',
      'n_gpus': N,
      'n_ranks_seen': _ranks_seen(),
      'dist_backend': ctx.dist_backend,
      'dataplane_selftest': getattr(ctx, 'selftest', None),
      'pg_timeout_s': getattr(ctx, 'pg_timeout', None),
      'steps': args.steps,
      'warmup': args.warmup,
      'ms_per_step': round(elapsed / args.steps * 1e3, 4),
      'higher_is_better': True,
      'scaling': 'strong' if args.strong else 'weak',
      'vs_baseline': None,
      'dtype': 'f32',
      'data': 'synthetic (counter-based splitmix64 U[0,1) / U[-1,1), resident in HBM)',
      'config': {'workload': 'cfg2: sum(x*y+exp(z), axis=0) + sum(x*y+exp(z), axis=1), x,y,z fp32 (%d,%d)'
                             % (R, S), 'shape': [R, S], 'tiling': 'row strips, one per rank (%d)' % N,
                 'parallelism': 'tile-dp%d' % N},
      'roofline': {'bound': 'hbm', 'achieved': round(achieved, 1) if achieved else None,
                   'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                   'frac': round(achieved / HBM_PEAK_GBS, 4) if achieved else None,
                   'traffic': traffic,
                   'traffic_source': 'profiles/%s (FETCH_SIZE/WRITE_SIZE passes)' % tname if traffic
                   else None,
                   'kernel': 'generated fused map+reduce: %s' % ' / '.join(knames),
                   'bytes_per_launch': bytes_launch,
                   'avg_launch_ms': round(avg * 1e3, 4) if red else None,
                   'axis0_ms': round(float(np.mean(ax0)) * 1e3, 4) if ax0 else None,
                   'axis1_ms': round(float(np.mean(ax1)) * 1e3, 4) if ax1 else None},
  }
  if args.dump_outputs:
    dump_outputs(args.dump_outputs, last, ctx)
  if not args.full:
    if ctx.rank == 0:
      print(json.dumps(result), flush=True)
    spartan_amd.shutdown()
    return
  result['checked'] = check_cfg2(last, x, y, z, R, S)
  result['cold_start'] = cold
  # SURVEY 8(d) cfg2 also: axis=None, and the materialised map (16 B/elem)
  result['cfg2_axis_none'] = bench_cfg2_extra('none', X, Y, Z, x, y, z, R, S, rows_local, be, expr, comm, sync)
  result['cfg2_map'] = bench_cfg2_extra('map', X, Y, Z, x, y, z, R, S, rows_local, be, expr, comm, sync)
  del x, y, z, X, Y, Z, last
  torch.cuda.empty_cache()
  result['vendor_reduce'] = vendor_reduce(achieved)
  torch.cuda.empty_cache()

  def leg(fn, *a):
    # a failing secondary leg is reported in the line, not allowed to take
    # the cfg2 headline down with it; each leg starts from a clean host state
    import gc
    from spartan_amd.expr.base import eval_cache
    eval_cache.clear()
    gc.collect()
    try:
      return fn(*a)
    except Exception as e:  # noqa: BLE001
      torch.cuda.empty_cache()
      return {'error': '%s: %s' % (type(e).__name__, str(e)[:300])}

  # the streaming legs before the GEMM leg: run after ~15 s of full-power
  # GEMMs, the HBM-bound lreg kernel measured 3.90-3.96 ms per iteration
  # against 3.79 on its own (gpurun_out/r4al vs r4am, round 4)
  wl = {'1': ('lreg', 'kmeans', 'kmeans_api'), '0': ()}.get(args.workloads, tuple(args.workloads.split(',')))
  dot_first = os.environ.get('SPARTAN_BENCH_DOT_FIRST') == '1'  # (dev A/B of the leg order)
  if args.dot and dot_first:
    result['dot'] = leg(bench_dot, args.dot_size, ctx, be, expr, comm, sync)
  if 'lreg' in wl:
    result['lreg'] = leg(bench_lreg, args.lreg_points, ctx, expr, comm, sync)
  if 'kmeans' in wl:
    result['kmeans'] = leg(bench_kmeans, args.km_points, ctx, expr, comm, sync)
  if 'kmeans_api' in wl:
    result['kmeans_api'] = leg(bench_kmeans_api, args.km_points, ctx, expr, comm, sync)

  if args.dot and not dot_first:
    result['dot'] = leg(bench_dot, args.dot_size, ctx, be, expr, comm, sync)

  if args.cpu_baseline and N == 1 and ctx.rank == 0:
    # the reference's multi-worker CPU model on this box's host cores
    # (oracle/cpu_baseline.py; bounded samples, about 30 s in all)
    from oracle import cpu_baseline as CB
    cb = CB.cfg2_cpu_baseline(rows=min(args.cpu_rows, S), cols=S, reps=5)
    out = {k: cb[k] for k in ('value', 'unit', 'cores', 'kind', 'sample', 'single_process', 'host')}
    out['value'] = round(cb['value'], 3)
    legs = {}
    # the side legs run on samples; each states its scale factor to the
    # BASELINE.json size and the time projected there at the sample's rate
    # (linear in N for lreg / k-means, the GFLOP/s held for the S^3 dot)
    sized = (('dot', CB.dot_cpu_baseline, {'S': 4096}, '32768 x 32768 fp32 (configs[3])', (32768 / 4096) ** 3),
             ('lreg', CB.lreg_cpu_baseline, {'N': 20_000_000}, '1e8 x 64 fp32 (configs[4])', 1e8 / 20_000_000),
             ('kmeans', CB.kmeans_cpu_baseline, {'N': 1_000_000}, '1e8 x 128 fp32, k=256 (configs[2])',
              1e8 / 1_000_000))
    for name, fn, kw, full, factor in sized:
      try:
        legs[name] = fn(**kw)
        lg = legs[name]
        lg['baseline_size'] = full
        lg['scale_to_baseline'] = factor
        if name == 'dot':
          lg['projected_seconds_at_baseline'] = round(2.0 * 32768 ** 3 / (lg['value'] * 1e9), 1)
        else:
          lg['projected_ms_per_iter_at_baseline'] = round(lg['ms_per_iter'] * factor, 1)
      except Exception as e:  # noqa: BLE001  (a failing side leg is reported, not fatal)
        legs[name] = {'error': '%s: %s' % (type(e).__name__, str(e)[:200])}
    out['legs'] = legs
    result['cpu_baseline'] = out
  if ctx.rank == 0:
    print(json.dumps(result), flush=True)
  spartan_amd.shutdown()
  failed = [k for k, v in result.items() if k == 'checked' and v is not True] + [
      k for k, v in result.items() if isinstance(v, dict) and v.get('checked') is False]
  if failed:
    sys.stderr.write('bench.py: post-timing validation FAILED for %s\n' % ', '.join(failed))
    sys.exit(3)


def dump_outputs(dirname, last, ctx):
  """What the timed path returned in its last step: the axis-0 sums (one per
  column) and the axis-1 sums (one per row of the global array), as float32
  .npy files.  Every rank takes part in the gather; rank 0 writes."""
  from spartan_amd.array import distarray
  arrays = {'axis0': distarray.glom(last[0]), 'axis1': distarray.glom(last[1])}
  if ctx.rank == 0:
    os.makedirs(dirname, exist_ok=True)
    for name, a in arrays.items():
      np.save(os.path.join(dirname, name + '.npy'), np.ascontiguousarray(a, dtype=np.float32))


# ------------------------------------------------------------------ checks
# Every leg validates the outputs it timed, after the timed region, against an
# independent fp64 restatement on a sample (host NumPy on glom'd rows /
# columns, or torch fp64 on the device tensors -- a checker, never the measured
# path).  A failed check prints the line with "checked": false and exits 3.
def _rel_ok(got, want, tol, scale=None):
  got = np.asarray(got, dtype=np.float64)
  want = np.asarray(want, dtype=np.float64)
  sc = np.abs(want) if scale is None else np.asarray(scale, dtype=np.float64)
  return bool(np.all(np.abs(got - want) <= tol * np.maximum(sc, 1e-300)))


def check_cfg2(last, x, y, z, R, S):
  """axis-1 results of three sampled rows and axis-0 results of three sampled
  columns against fp64 sums of the same fp32 inputs; sum of the axis-0
  result against the sum of the axis-1 result.  Tolerance 1e-5 relative
  (the north star's fp32 bound)."""
  from spartan_amd.array import distarray, extent as ext
  a0, a1 = last
  g0 = distarray.glom(a0).astype(np.float64)
  g1 = distarray.glom(a1).astype(np.float64)
  ok = _rel_ok(g0.sum(), g1.sum(), 1e-5)
  for i in (0, R // 3, R - 1):
    reg = ext.create((i, 0), (i + 1, S), (R, S))
    xr, yr, zr = (distarray.glom_region(t, reg).astype(np.float64).ravel() for t in (x, y, z))
    ok &= _rel_ok(g1[i], np.sum(xr * yr + np.exp(zr)), 1e-5)
  for j in (0, S // 2 + 1, S - 1):
    reg = ext.create((0, j), (R, j + 1), (R, S))
    xc, yc, zc = (distarray.glom_region(t, reg).astype(np.float64).ravel() for t in (x, y, z))
    ok &= _rel_ok(g0[j], np.sum(xc * yc + np.exp(zc)), 1e-5)
  return bool(ok)


def vendor_reduce(achieved, n=1 << 30, runs=10):
  """The same box's vendor reduction for comparison: ATen's torch.sum over one
  2^30 fp32 tensor (4 GiB), HIP events on torch's stream, median of ``runs``.
  ``cfg2_over_vendor`` = the cfg2 kernel's rate / this one (a comparison
  point, not a ceiling: the read-stream ceiling of these boxes is 7.0-7.4
  TB/s, profiles/r02_stream_ceiling_before.txt)."""
  import torch
  t = torch.empty(n, dtype=torch.float32, device='cuda').uniform_()
  for _ in range(2):
    t.sum()
  torch.cuda.synchronize()
  ms = []
  for _ in range(runs):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    t.sum()
    b.record()
    b.synchronize()
    ms.append(a.elapsed_time(b))
  del t
  torch.cuda.empty_cache()
  med = float(np.median(ms))
  gbs = 4.0 * n / (med * 1e-3) / 1e9
  return {'kernel': 'torch.sum over one 2^30 fp32 tensor (ATen reduce)', 'ms': round(med, 4), 'GBps': round(gbs, 1),
          'frac': round(gbs / HBM_PEAK_GBS, 4),
          'cfg2_over_vendor': round(achieved / gbs, 4) if achieved else None}


def _ranks_seen():
  import torch.distributed as dist
  return dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1


def cold_start(expr, X, Y, Z, sync):
  """First evaluation in the process of sum(x*y+exp(z), axis=0).optimized()
  .force() (DAG rewrite, plan, codegen, code-object load from the build()-time
  cache, module load, the kernel itself), the second one (steady state: plan
  replay, kernel), and the device compiler's time for that kernel's source
  when it is in no cache (a salted copy, compiled into a temporary cache)."""
  import tempfile
  from spartan_amd import backend, codegen
  from spartan_amd.config import FLAGS
  out = {}
  for k in ('first_eval_ms', 'second_eval_ms'):
    sync()
    t0 = time.perf_counter()
    expr.sum(X * Y + expr.exp(Z), axis=0).optimized().force()
    sync()
    out[k] = round((time.perf_counter() - t0) * 1e3, 3)
  f32 = np.dtype(np.float32)
  In, Op = codegen.In, codegen.Op
  tree = Op('add', [Op('multiply', [In(0, f32), In(1, f32)]), Op('exp', [In(2, f32)])])
  src, _ = codegen.named(codegen.gen_reduce(tree, [(0, f32), (1, f32), (2, f32)], ['c'] * 3, 'cols', 'sum',
                                            codegen.vec_width([f32])), 'spx_reduce', 'cols')
  prev = FLAGS.kernel_cache_dir
  try:
    with tempfile.TemporaryDirectory() as td:
      FLAGS.kernel_cache_dir = td
      t0 = time.perf_counter()
      backend.compile_code_object(src + '\n// cold-start probe %d %f\n' % (os.getpid(), time.time()))
      out['compile_ms'] = round((time.perf_counter() - t0) * 1e3, 1)
  except Exception as e:  # noqa: BLE001  (no device compiler: report, do not fail the bench)
    out['compile_ms'] = None
    out['compile_error'] = '%s: %s' % (type(e).__name__, str(e)[:200])
  finally:
    FLAGS.kernel_cache_dir = prev
  out['note'] = ('first_eval_ms: the first .optimized().force() of the cfg2 axis-0 sum in this process (kernel '
                 'from the build()-time code-object cache); compile_ms: device clang for that source uncached')
  return out


def bench_cfg2_extra(kind, X, Y, Z, x, y, z, R, S, rows_local, be, expr, comm, sync, steps=10, warm=2):
  """SURVEY 8(d) cfg2 extras: 'none' = sum(x*y+exp(z)) over all elements
  (per-rank partial, all-reduce; 12 B/elem), 'map' = the materialised map
  (x*y+exp(z)).optimized().force() (16 B/elem: three reads, one write).
  Wall time over ``steps`` evaluations (barrier + synchronize on both
  sides, max over ranks) and the generated kernel's HIP-event time."""
  import torch

  def ev():
    if kind == 'none':
      return expr.sum(X * Y + expr.exp(Z)).optimized().force()
    return (X * Y + expr.exp(Z)).optimized().force()
  for _ in range(warm):
    r = ev()
    del r
  sync()
  comm.barrier()
  sync()
  be.kernel_events = []
  t0 = time.perf_counter()
  for _ in range(steps):
    r = ev()
    if kind == 'map':
      last = r
    del r
  sync()
  comm.barrier()
  sync()
  el = comm.max_over_ranks(time.perf_counter() - t0)
  events = be.kernel_events
  be.kernel_events = None
  pre = 'spx_reduce' if kind == 'none' else 'spx_map'
  ks = [s_.elapsed_time(e_) * 1e-3 for (n, s_, e_) in events if n.startswith(pre)]
  per_elem = 12 if kind == 'none' else 16
  nbytes = per_elem * R * S
  blaunch = per_elem * rows_local * S
  kavg = float(np.mean(ks)) if ks else None
  out = {'GBps': round(nbytes * steps / el / 1e9, 1), 'ms_per_eval': round(el / steps * 1e3, 4),
         'kernel_ms': round(kavg * 1e3, 4) if kavg else None,
         'roofline': {'bound': 'hbm', 'achieved': round(blaunch / kavg / 1e9, 1) if kavg else None,
                      'peak': HBM_PEAK_GBS, 'unit': 'GB/s',
                      'frac': round(blaunch / kavg / 1e9 / HBM_PEAK_GBS, 4) if kavg else None,
                      'bytes_per_launch': blaunch,
                      'kernel': ' / '.join(sorted({n for (n, _, _) in events if n.startswith(pre)}))}}
  if kind == 'none':
    want = None
    got = float(expr.sum(X * Y + expr.exp(Z)).optimized().glom())
    # against the (already checked) axis-1 sums, summed in fp64
    want = float(expr.sum(expr.astype(expr.sum(X * Y + expr.exp(Z), axis=1), np.float64)).glom())
    out['checked'] = _rel_ok(got, want, 1e-5)
    out['config'] = 'sum(x*y+exp(z)) (axis=None), %d x %d fp32' % (R, S)
  else:
    from spartan_amd.array import distarray, extent as ext
    ok = True
    for i in (0, R // 2, R - 1):
      reg = ext.create((i, 0), (i + 1, S), (R, S))
      xr, yr, zr = (distarray.glom_region(t, reg).astype(np.float64).ravel() for t in (x, y, z))
      got = distarray.glom_region(last, reg).astype(np.float64).ravel()
      ok &= _rel_ok(got, xr * yr + np.exp(zr), 1e-6)
    out['checked'] = bool(ok)
    out['config'] = '(x*y+exp(z)).optimized().force(): materialised (%d, %d) fp32 result' % (R, S)
    del last
  torch.cuda.empty_cache()
  return out


def _kernel_ms(events, prefix):
  ks = [s_.elapsed_time(e_) for (n, s_, e_) in events if n.startswith(prefix)]
  return float(np.mean(ks)) if ks else None


def bench_dot(S, ctx, be, expr, comm, sync, runs=10, warm=2):
  """dot(A, B) for S x S fp32 and fp64 (configs[3]); GFLOP/s over all ranks.
  SURVEY.md 8(d): median of ``runs`` timed evaluations after ``warm``
  warm-ups, each bracketed by barrier + synchronize, max over ranks."""
  import torch
  out = {}
  for dt, peak in ((np.float32, MFMA_F32_TFS), (np.float64, MFMA_F64_TFS)):
    a = expr.rand(S, S, dtype=dt, seed=31).force()
    b = expr.rand(S, S, dtype=dt, seed=32).force()
    A, B = expr.lazify(a), expr.lazify(b)
    for _ in range(warm):  # JIT-free: spx_gemm is ahead-of-time
      c = expr.dot(A, B).force()
      del c
    times = []
    be.kernel_events = []
    for _ in range(runs):
      sync()
      comm.barrier()
      sync()
      t0 = time.perf_counter()
      c = expr.dot(A, B).force()
      sync()
      comm.barrier()
      sync()
      times.append(comm.max_over_ranks(time.perf_counter() - t0))
      if len(times) < runs:
        del c
    events = be.kernel_events
    be.kernel_events = None
    gemm_ms = [s_.elapsed_time(e_) for (n, s_, e_) in events if n == 'spx_gemm']
    checked = check_dot(c, A, B, S, dt, expr)
    del c
    el = float(np.median(times))
    flops = 2.0 * S ** 3
    name = 'f32' if dt == np.float32 else 'f64'
    out[name] = {'gflops': round(flops / el / 1e9, 1), 'seconds': round(el, 4),
                 'seconds_min_max': [round(min(times), 4), round(max(times), 4)],
                 'mfma_frac_per_gpu': round(flops / el / 1e12 / (peak * ctx.world_size), 4),
                 'checked': checked}
    if gemm_ms and ctx.world_size == 1:
      # the dominant kernel alone: spx_gemm's HIP-event time per dot (one call per dot at N = 1)
      km = float(np.sum(gemm_ms)) / runs
      out[name]['kernel_ms'] = round(km, 3)
      out[name]['kernel_mfma_frac'] = round(flops / (km * 1e-3) / 1e12 / peak, 4)
    if ctx.world_size == 1 and os.environ.get('SPARTAN_BENCH_VENDOR_GEMM', '1') != '0':
      try:
        out[name]['vendor'] = vendor_gemm(a, b, S, peak, out[name].get('kernel_ms'))
      except Exception as e:  # noqa: BLE001  (a comparison point: reported, not fatal)
        out[name]['vendor'] = {'error': '%s: %s' % (type(e).__name__, str(e)[:200])}
    del a, b, A, B
    torch.cuda.empty_cache()
  out['config'] = ('dot(A, B), A, B ~ U[0,1) (%d, %d), K-split over ranks; median of %d runs after %d warm-ups'
                   % (S, S, runs, warm))
  return out


def vendor_gemm(a, b, S, peak, ours_ms, runs=5, warm=2):
  """The same box's vendor GEMM on the same resident operands: torch.matmul
  (hipBLASLt / rocBLAS through ATen; TF32-style reduced precision off, so
  fp32 is computed in fp32), HIP events on torch's stream, median of
  ``runs`` after ``warm`` warm-ups.  ``ours_over_vendor`` = the vendor's
  kernel time / spx_gemm's (> 1: ours is faster)."""
  import torch
  ta = next(iter(a.local.values())).data
  tb = next(iter(b.local.values())).data
  assert tuple(ta.shape) == (S, S) and tuple(tb.shape) == (S, S)
  prev = torch.backends.cuda.matmul.allow_tf32
  torch.backends.cuda.matmul.allow_tf32 = False
  try:
    c = torch.empty((S, S), dtype=ta.dtype, device=ta.device)
    for _ in range(warm):
      torch.matmul(ta, tb, out=c)
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
      e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      e0.record()
      torch.matmul(ta, tb, out=c)
      e1.record()
      e1.synchronize()
      ms.append(e0.elapsed_time(e1))
    del c
  finally:
    torch.backends.cuda.matmul.allow_tf32 = prev
    torch.cuda.empty_cache()
  med = float(np.median(ms))
  tf = 2.0 * S ** 3 / (med * 1e-3) / 1e12
  return {'kernel': 'torch.matmul (ATen -> hipBLASLt / rocBLAS), allow_tf32=False', 'ms': round(med, 3),
          'ms_min_max': [round(min(ms), 3), round(max(ms), 3)], 'tflops': round(tf, 1),
          'mfma_frac': round(tf / peak, 4),
          'ours_over_vendor': round(med / ours_ms, 4) if ours_ms else None}


def check_dot(c, A, B, S, dt, expr):
  """Row sums of two sampled rows of C = A B against A[i, :] . (B 1) and
  column sums of two sampled columns against (1^T A) . B[:, j], the vectors
  B 1 and 1^T A taken in fp64 by the reduction kernels (not the GEMM);
  tolerance 1e-5 (fp32) / 1e-11 (fp64) relative to the fp64 sums of |terms|."""
  from spartan_amd.array import distarray, extent as ext
  tol = 1e-5 if dt == np.float32 else 1e-11
  b1 = expr.sum(expr.astype(B, np.float64), axis=1).glom()
  a1 = expr.sum(expr.astype(A, np.float64), axis=0).glom()
  ok = True
  for i in (1, S - 2):
    ar = distarray.glom_region(A.force(), ext.create((i, 0), (i + 1, S), (S, S))).astype(np.float64).ravel()
    cr = distarray.glom_region(c, ext.create((i, 0), (i + 1, S), (S, S))).astype(np.float64).ravel()
    ok &= _rel_ok(cr.sum(), ar @ b1, tol, np.abs(ar) @ np.abs(b1))
  for j in (2, S - 3):
    bc = distarray.glom_region(B.force(), ext.create((0, j), (S, j + 1), (S, S))).astype(np.float64).ravel()
    cc = distarray.glom_region(c, ext.create((0, j), (S, j + 1), (S, S))).astype(np.float64).ravel()
    ok &= _rel_ok(cc.sum(), a1 @ bc, tol, np.abs(a1) @ np.abs(bc))
  return bool(ok)


def check_kmeans(X, labels, centers, comm, n_check=1 << 20, dist_dtype=np.float64):
  """The labels of the first n_check local rows against the all-exact
  assignment kernel (scipy cdist order for every point and centre; the
  distances rounded to dist_dtype first, as the reference's outer target
  does for the drop-in loop): bit for bit."""
  import torch
  from spartan_amd import backend, runtime
  be = backend.get()
  ctx = runtime.get()
  cdev = torch.as_tensor(np.ascontiguousarray(centers, dtype=np.float64)).to(ctx.device)
  ok = True
  for ex, tile in X.local.items():
    n = min(n_check, ex.shape[0])
    lab = labels.local[[e for e in labels.local if e.ul[0] == ex.ul[0]][0]].data[:n]
    want = torch.empty((n,), dtype=torch.int64, device=ctx.device)
    be.kmeans_assign(tile.data[:n], cdev, want, exact_only=True, dist_dtype=dist_dtype)
    ok &= bool(torch.equal(lab, want))
  return bool(comm.max_over_ranks(0.0 if ok else 1.0) == 0.0)


def check_kmeans_sums(X, labels, sums, counts, comm, chunk=1 << 20):
  """The last iteration's all-reduced counts against the bincount of its
  labels (exact), and its centre sums against an fp64 index-add of the same
  rows (torch fp64 on the device, a checker only), all-reduced over ranks:
  every element within 1e-5 of the sum of |x| of its centre's rows."""
  import torch
  from spartan_amd import runtime
  ctx = runtime.get()
  K, D = sums.shape
  ws = torch.zeros((K, D), dtype=torch.float64, device=ctx.device)
  wa = torch.zeros((K, D), dtype=torch.float64, device=ctx.device)
  wc = torch.zeros((K,), dtype=torch.int64, device=ctx.device)
  for ex, tile in X.local.items():
    lab = labels.local[[e for e in labels.local if e.ul[0] == ex.ul[0]][0]].data
    for r0 in range(0, ex.shape[0], chunk):
      # one-hot fp64 GEMMs, not index_add_ (its fp64 atomics serialise when
      # most rows share a label, as a first iteration's may)
      lb = lab[r0:r0 + chunk]
      oh = torch.nn.functional.one_hot(lb, K).to(torch.float64).t()
      xb = tile.data[r0:r0 + chunk].to(torch.float64)
      ws += oh @ xb
      wa += oh @ xb.abs()
      wc += torch.bincount(lb, minlength=K)
  comm.all_reduce(ws, 'sum')
  comm.all_reduce(wa, 'sum')
  comm.all_reduce(wc, 'sum')
  ok = bool(np.array_equal(wc.cpu().numpy(), np.asarray(counts)))
  ok &= bool(np.all(np.abs(np.asarray(sums) - ws.cpu().numpy()) <= 1e-5 * wa.cpu().numpy() + 1e-300))
  return ok


def bench_kmeans(npts, ctx, expr, comm, sync, D=128, K=256, iters=2):
  """configs[2]: one k-means iteration (spx_kmeans_step: the certified
  fp16 screen fused with the centroid accumulation, bf16x3 / exact-order
  passes over its undecided rows = scipy-exact labels, fp32 window sums
  combined in fp64, all-reduce) over npts x 128 fp32 points, k=256.
  Checked after the timed region: labels (a 1 M-row prefix, bit for bit),
  counts (exact) and sums (1e-5 of sum |x|) of the last iteration."""
  import torch
  from spartan_amd import workloads
  from spartan_amd.array import distarray, extent as ext
  X = expr.rand(npts * ctx.world_size, D, dtype=np.float32, seed=21).force()
  # the first K points as the initial centres, read before the timed region
  # (as the API leg does: both legs time the same iterations)
  c0 = distarray.glom_region(X, ext.create((0, 0), (K, D), X.shape)).astype(np.float64)
  workloads.kmeans_fit(X, K, iters, centers=c0)      # warm-up (every path of the timed loop)
  from spartan_amd import backend
  be = backend.get()
  be.kmeans_timing(True)  # HIP events around the one-pass kernel of each step (no host sync inside)
  try:
    sync()
    comm.barrier()
    t0 = time.perf_counter()
    info = {}
    c, labels = workloads.kmeans_fit(X, K, iters, centers=c0, info=info)
    sync()
    comm.barrier()
    el = comm.max_over_ranks(time.perf_counter() - t0) / iters
    kt = be.kmeans_times()
  finally:
    be.kmeans_timing(False)
  checked = check_kmeans(X, labels, info['assign_centers'], comm)
  checked_sums = check_kmeans_sums(X, labels, info['sums'], info['counts'], comm)
  n = npts * ctx.world_size
  out = {'ms_per_iter': round(el * 1e3, 3), 'points_per_s': round(n / el, 1),
         'gemm_form_tflops': round(2.0 * n * K * D / el / 1e12, 2),
         # the screen runs the distance GEMM once on fp16 MFMAs (the bf16x3
         # pass re-runs only its few % undecided rows), so the GEMM-form rate
         # over the dense fp16/bf16 peak is its matrix-core share of the whole
         # iteration; the fused step reads X once (4 N D bytes; FETCH_SIZE:
         # 1.16 x that, profiles/r03_kmeans_step_pmc.json)
         'f16_mfma_frac_per_gpu': round(2.0 * n * K * D / el / 1e12 / (2500.0 * ctx.world_size), 4),
         'hbm_GBps_one_pass': round(4.0 * n * D / el / 1e9, 1),
         'checked': checked and checked_sums, 'checked_labels': checked, 'checked_sums_counts': checked_sums,
         # iterations queued before the host read the previous counts (kept:
         # device quotients bit-identical to the host's, no empty cluster) /
         # queued again with the host's centres (workloads.kmeans_fit)
         'speculated_iters': info.get('speculated'), 'respun_iters': info.get('respun'),
         'kernel_ms': [round(a, 3) for a, _ in kt], 'step_ms': [round(b, 3) for _, b in kt],
         'host_overhead_ms_per_iter': (round(el * 1e3 - float(np.mean([b for _, b in kt])), 3) if kt else None),
         'kernel_hbm_frac': (round(4.0 * npts * D / (float(np.mean([a for a, _ in kt])) * 1e-3) / 1e9 / HBM_PEAK_GBS,
                                   4) if kt else None),
         'kernel_note': 'kernel_ms / step_ms: HIP events (spx_kmeans_timing) around k_kmeans_pp (the one-pass '
                        'screen + accumulation) and around the whole spx_kmeans_step, per iteration; '
                        'kernel_hbm_frac = the points (4 N D bytes, read once) / mean kernel_ms / 8 TB/s',
         'config': 'cfg3: %d x %d fp32 points (U[0,1), seed 21) per GPU, k=%d, centres = first %d points; '
                   'spx_kmeans_step: certified fp16-MFMA screen + per-centre sums of the rows it decides in one '
                   'pass over X, bf16x3-MFMA pass + exact-order fp64 recompute of its undecided rows (bit-exact '
                   'labels) + their gathered sums; centre sums in fp32 per block and window of 16128 rows, '
                   'the windows combined in fp64; iteration i + 1 queued with device-divided centres before '
                   'the host checks iteration i (kept only when bit-identical to the host division)'
                   % (npts, D, K, K)}
  del X, labels
  torch.cuda.empty_cache()
  return out


def bench_kmeans_api(npts, ctx, expr, comm, sync, D=128, K=256, iters=2):
  """configs[2] through the drop-in API: the reference's KMeans.fit loop
  (k_means_.py:125-152) -- expr.outer + expr.argmin (fused into the certified
  assignment), map2 bincount, map2 centre sums, host divide -- on the same
  points and initial centres as the direct-kernel leg."""
  import torch
  from spartan_amd.array import distarray, extent as ext
  from spartan_amd.examples.kmeans import KMeans
  X = expr.rand(npts * ctx.world_size, D, dtype=np.float32, seed=21).force()
  c0 = distarray.glom_region(X, ext.create((0, 0), (K, D), X.shape)).astype(np.float64)
  KMeans(K, iters).fit(X, c0)  # warm-up: as many iterations as the timed fit (the direct leg's warm-up too),
  # so the timed run meets a caching allocator that already holds two label buffers
  from spartan_amd import backend
  be = backend.get()
  be.kmeans_timing(True)  # the same per-step HIP events as the direct leg
  try:
    sync()
    comm.barrier()
    t0 = time.perf_counter()
    km = KMeans(K, iters)
    c_api, labels = km.fit(X, c0)
    sync()
    comm.barrier()
    el = comm.max_over_ranks(time.perf_counter() - t0) / iters
    kt = be.kmeans_times()
  finally:
    be.kmeans_timing(False)
  n = npts * ctx.world_size
  # the last iteration's labels against the all-exact assignment kernel with
  # the centres that iteration used (a prefix of each local row strip)
  ac = km.assign_centers_
  ac = ac.glom() if hasattr(ac, 'glom') else np.asarray(ac)
  checked = check_kmeans(X, labels.force() if hasattr(labels, 'force') else labels, ac, comm,
                         dist_dtype=X.dtype)  # kmeans_dist_mapper's target has the points' dtype
  out = {'ms_per_iter': round(el * 1e3, 3), 'points_per_s': round(n / el, 1), 'checked': checked,
         'step_ms': [round(b, 3) for _, b in kt],
         # the time per iteration outside the fused steps (HIP events around each
         # spx_kmeans_step): the loop's host round trip and glue, comparable with
         # the direct leg's figure whatever the clock does between the legs
         'host_overhead_ms_per_iter': (round(el * 1e3 - float(np.mean([b for _, b in kt])), 3) if kt else None),
         'config': 'cfg3 via examples.kmeans.KMeans(%d, %d).fit(X, first %d points): outer + argmin '
                   '(OuterArgminFusion -> certified assignment), map2 bincount, map2 centre sums' % (K, iters, K)}
  del X
  torch.cuda.empty_cache()
  return out


def check_lreg(Xe, Ye, w, expr, comm, chunk=1 << 23):
  """The fused gradient sum(x * (dot(x, w) - y), axis=0) at w against a chunked fp64 restatement over the local row strips (torch fp64
  on the device, a checker only), all-reduced over ranks: per column within
  1e-5 of sum_i |x_ij| |r_i| (the condition of the sum)."""
  import torch
  from spartan_amd import runtime
  ctx = runtime.get()
  g = expr.sum(Xe * (expr.dot(Xe, w) - Ye), axis=0).optimized().glom().astype(np.float64)
  X, Y = Xe.force(), Ye.force()
  D = X.shape[1]
  wd = torch.as_tensor(np.asarray(w, dtype=np.float64).reshape(D)).to(ctx.device)
  acc = torch.zeros((2, D), dtype=torch.float64, device=ctx.device)
  ytiles = {ex.ul[0]: t for ex, t in Y.local.items()}
  for ex, t in X.local.items():
    yt = ytiles[ex.ul[0]].data.reshape(-1)
    for r0 in range(0, ex.shape[0], chunk):
      xc = t.data[r0:r0 + chunk].to(torch.float64)
      res = torch.mv(xc, wd) - yt[r0:r0 + chunk].to(torch.float64)
      # (x^T r as a transposed GEMV: a (1 x n) @ (n x 64) product ran as an
      # fp64 GEMM at ~0.28 s per chunk, 40x the GEMV)
      acc[0] += torch.mv(xc.t(), res)
      acc[1] += torch.mv(xc.abs().t(), res.abs())
      del xc, res
  comm.all_reduce(acc, 'sum')
  ref = acc.cpu().numpy()
  return _rel_ok(g, ref[0], 1e-5, ref[1])


def bench_lreg(npts, ctx, expr, comm, sync, D=64, iters=30):
  """configs[4]: linear-regression gradient step X^T(Xw - y) + all-reduce."""
  import torch
  from spartan_amd import workloads
  X = expr.rand(npts * ctx.world_size, D, dtype=np.float32, seed=41).force()
  Y = expr.rand(npts * ctx.world_size, 1, dtype=np.float32, seed=42).force()
  w = np.random.default_rng(43).random((D, 1)).astype(np.float32)
  Xe, Ye = expr.lazify(X), expr.lazify(Y)
  workloads.sgd_train(Xe, Ye, w, 1e-6, 2)  # warm-up (kernel compile / load, plan caches)
  from spartan_amd import backend
  be = backend.get()
  sync()
  comm.barrier()
  be.kernel_events = []
  t0 = time.perf_counter()
  w_end = workloads.sgd_train(Xe, Ye, w, 1e-6, iters)
  sync()
  comm.barrier()
  el = comm.max_over_ranks(time.perf_counter() - t0) / iters
  events = be.kernel_events
  be.kernel_events = None
  # the fused gradient kernel (generated spx_reduce_cols_*) and every kernel of the iteration
  kred = _kernel_ms(events, 'spx_reduce')
  kall = sum(s_.elapsed_time(e_) for (_, s_, e_) in events) / iters
  # checked at the starting w: the reference's step size (sgd.py:14, alpha =
  # 1e-6) diverges at this N, so after 30 steps w and the gradient have left
  # the fp32 range; the replayed plan and kernel are the ones timed
  checked = check_lreg(Xe, Ye, w, expr, comm)
  del w_end
  n = npts * ctx.world_size
  nbytes = 4.0 * n * D + 4.0 * n   # one pass: X and y read once (DotReduceFusion)
  nloc = nbytes / ctx.world_size
  out = {'ms_per_iter': round(el * 1e3, 3), 'algorithmic_GBps': round(nbytes / el / 1e9, 1),
         'hbm_frac_per_gpu': round(nbytes / el / 1e9 / (HBM_PEAK_GBS * ctx.world_size), 4),
         'kernel_ms': round(kred, 4) if kred else None,
         'kernel_hbm_frac': round(nloc / (kred * 1e-3) / 1e9 / HBM_PEAK_GBS, 4) if kred else None,
         'device_ms_per_iter': round(kall, 4),
         'kernel_note': 'kernel_ms: HIP events around the fused gradient kernel (X and y read once: 4 N (d + 1) '
                        'bytes); device_ms_per_iter: every kernel of an iteration (gradient, finalize, w update); '
                        'ms_per_iter - device_ms_per_iter = launch gaps and host work',
         'checked': checked,
         'config': 'cfg5: X %d x %d fp32, y %d x 1, w 64 x 1 (device-resident between iterations, '
                   'w - grad * alpha as a device map: no per-iteration host round trip); grad = sum(x * (dot(x, '
                   'w) - y), axis=0): dot folded into the fused axis-0 reduction (one pass over X) + all-reduce of '
                   '64 fp32' % (n, D, n)}
  del X, Y, Xe, Ye
  torch.cuda.empty_cache()
  return out


if __name__ == '__main__':
  main()
