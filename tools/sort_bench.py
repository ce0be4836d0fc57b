"""Measure ``spartan_amd.sort`` / ``argsort`` (spx_sort) against torch.sort on
one GPU.

Configurations (fp32): a (32768, 32768) array along axis 1 and axis 0 (radix
path, contiguous and strided lines), a 1-d array of 2^28 elements (one long
line) and a (2^20, 256) array along axis 1 (the LDS path).  Each is timed with
HIP events over 20 steps after 5 warm-up steps of ``expr.sort(X, axis)
.force()`` and of ``expr.argsort(X, axis).force()``; in the same process
``torch.sort(t, dim=axis, stable=True)`` (which returns values and indices) runs
on the same device tensor as the vendor figure.  ``kernel_ms`` is spx_sort
alone on preallocated outputs (HipBackend.sort).

Every configuration runs in a child process of its own under
``timeout -k 10``; after a failed child nothing more is started.  Prints one
JSON line (and writes it to --out).

  python tools/sort_bench.py --out profiles/sort_bench_<tag>.json
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = ['axis1', 'axis0', 'flat1d', 'short']
WARMUP, STEPS = 5, 20


def _time(fn):
  import torch
  for _ in range(WARMUP):
    fn()
  torch.cuda.synchronize()
  evs = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(STEPS)]
  for a, b in evs:
    a.record()
    fn()
    b.record()
  torch.cuda.synchronize()
  ms = sorted(a.elapsed_time(b) for a, b in evs)
  return sum(ms) / len(ms), ms[len(ms) // 2], ms[0], ms[-1]


def run_config(name, small):
  import numpy as np
  import torch
  import spartan_amd
  from spartan_amd import backend, expr
  spartan_amd.initialize()
  be = backend.get()
  assert isinstance(be, backend.HipBackend)
  if name == 'flat1d':
    shape, axis = ((1 << 16,) if small else (1 << 28,)), 0
  elif name == 'short':
    shape, axis = ((1 << 10, 256) if small else (1 << 20, 256)), 1
  else:
    shape = (512, 4096) if small else (32768, 32768)
    axis = {'axis0': 0, 'axis1': 1}[name]
  x = expr.rand(*shape, dtype=np.float32, seed=17).force()
  (ex, tile), = x.local.items()  # one worker: the whole array is one tile
  t = tile.data
  X = expr.lazify(x)
  N = int(np.prod(shape))
  geom = (int(np.prod(shape[:axis])), shape[axis], int(np.prod(shape[axis + 1:])))
  path, passes = backend.sort_plan(geom[0], geom[1], geom[2], np.float32)
  vals = torch.empty(shape, dtype=torch.float32, device=t.device)
  idx = torch.empty(shape, dtype=torch.int64, device=t.device)

  res = {'config': name, 'shape': list(shape), 'axis': axis, 'path': path, 'passes': passes}
  for what, ours, kernel in (
      ('sort', lambda: expr.sort(X, axis=axis).force(), lambda: be.sort(t, vals, None, geom)),
      ('argsort', lambda: expr.argsort(X, axis=axis).force(), lambda: be.sort(t, None, idx, geom))):
    mean, med, best, worst = _time(ours)
    kmean = _time(kernel)[0]
    res[what] = {'ms': round(mean, 4), 'ms_median': round(med, 4), 'ms_min': round(best, 4),
                 'ms_max': round(worst, 4), 'kernel_ms': round(kmean, 4),
                 'gkeys_per_s': round(N / (mean / 1e3) / 1e9, 3)}
  vmean, vmed, vbest, vworst = _time(lambda: torch.sort(t, dim=axis, stable=True))
  res['torch_sort_stable'] = {'ms': round(vmean, 4), 'ms_median': round(vmed, 4), 'ms_min': round(vbest, 4),
                              'ms_max': round(vworst, 4), 'gkeys_per_s': round(N / (vmean / 1e3) / 1e9, 3)}
  for what in ('sort', 'argsort'):
    res[what]['ours_over_torch'] = round(res[what]['ms'] / vmean, 3)
  # the two agree: the data has no NaN and no zeros of both signs, so bit for bit
  tv, ti = torch.sort(t, dim=axis, stable=True)
  res['values_equal_torch'] = bool(torch.equal(expr.sort(X, axis=axis).force().local[ex].data, tv))
  res['indices_equal_torch'] = bool(torch.equal(expr.argsort(X, axis=axis).force().local[ex].data, ti))
  return res


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--config', choices=CONFIGS, help='run one configuration in this process (child mode)')
  ap.add_argument('--small', action='store_true', help='toy sizes (a rehearsal of the script, not a measurement)')
  ap.add_argument('--timeout', type=int, default=240, help='seconds per configuration')
  ap.add_argument('--out', help='also write the JSON line to this file')
  args = ap.parse_args()
  if args.config:
    print('SORT_BENCH ' + json.dumps(run_config(args.config, args.small)), flush=True)
    return 0
  results, failed = [], None
  for name in CONFIGS:
    cmd = ['timeout', '-k', '10', str(args.timeout), sys.executable, os.path.abspath(__file__), '--config', name]
    if args.small:
      cmd.append('--small')
    r = subprocess.run(cmd, capture_output=True, text=True)
    line = [l for l in r.stdout.splitlines() if l.startswith('SORT_BENCH ')]
    if r.returncode != 0 or not line:
      failed = {'config': name, 'exit': r.returncode, 'stderr': r.stderr[-2000:]}
      break  # nothing more is started on the GPU after a failure
    results.append(json.loads(line[-1][len('SORT_BENCH '):]))
  doc = {'tool': 'sort_bench', 'dtype': 'float32', 'warmup': WARMUP, 'steps': STEPS, 'small': bool(args.small),
         'configs': results}
  if failed:
    doc['failed'] = failed
  text = json.dumps(doc)
  print(text, flush=True)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(text + '\n')
  return 1 if failed else 0


if __name__ == '__main__':
  sys.exit(main())
