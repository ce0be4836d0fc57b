"""Measure ``spartan_amd.scan`` (spx_scan) against torch.cumsum on one GPU.

Configurations (fp32): scan of a (32768, 32768) array along axis 0, axis 1
and axis None, and of a 1-d array of 2^28 elements.  Each is timed with HIP
events over 20 steps after 5 warm-up steps, and in the same process
torch.cumsum runs on the same device tensor as the vendor figure.  GB/s is
over the algorithmic 2 * N * 4 bytes (one read, one write), whatever the
kernel mode really moves.

Every configuration runs in a child process of its own under
``timeout -k 10``; after a failed child nothing more is started.  Prints one
JSON line (and writes it to --out).

  python tools/scan_bench.py --out profiles/scan_bench_<tag>.json
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = ['axis0', 'axis1', 'axisNone', 'flat1d']
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
  return sum(ms) / len(ms), ms[len(ms) // 2], ms[0]


def run_config(name, small):
  import numpy as np
  import torch
  import spartan_amd
  from spartan_amd import backend, expr
  spartan_amd.initialize()
  assert isinstance(backend.get(), backend.HipBackend)
  if name == 'flat1d':
    shape, axis = ((1 << 16,) if small else (1 << 28,)), 0
  else:
    shape = (512, 512) if small else (32768, 32768)
    axis = {'axis0': 0, 'axis1': 1, 'axisNone': None}[name]
  x = expr.rand(*shape, dtype=np.float32, seed=17).force()
  (ex, tile), = x.local.items()  # one worker: the whole array is one tile
  t = tile.data
  X = expr.lazify(x)
  N = int(np.prod(shape))
  if axis is None:
    geom = (int(np.prod(shape[:-1])), shape[-1], 1)  # the per-tile passes (totals, then the scan with its bases)
  else:
    geom = (int(np.prod(shape[:axis])), shape[axis], int(np.prod(shape[axis + 1:])))
  mode = backend.scan_plan(geom[0], geom[1], geom[2], np.float32)[0]

  def ours():
    expr.scan(X, axis=axis).force()

  def vendor():
    torch.cumsum(t.reshape(-1) if axis is None else t, 0 if axis is None else axis)

  mean, med, best = _time(ours)
  vmean, vmed, vbest = _time(vendor)
  # the two agree (fp32 results of an fp64-accumulated scan vs the vendor's)
  got = expr.scan(X, axis=axis).force().local[ex].data
  want = torch.cumsum((t.reshape(-1) if axis is None else t).double(), 0 if axis is None else axis).float().reshape(shape)
  same = bool(torch.equal(got, want))
  maxrel = float(((got - want).abs() / want.abs().clamp_min(1e-30)).max().item())
  gb = 2.0 * N * 4 / 1e9
  return {'config': name, 'shape': list(shape), 'axis': axis, 'mode': mode, 'ms': round(mean, 4),
          'ms_median': round(med, 4), 'ms_min': round(best, 4), 'gbps': round(gb / (mean / 1e3), 1),
          'torch_cumsum_ms': round(vmean, 4), 'torch_cumsum_ms_median': round(vmed, 4),
          'torch_cumsum_gbps': round(gb / (vmean / 1e3), 1), 'speedup_vs_torch': round(vmean / mean, 3),
          'equals_fp64_cumsum_rounded': same, 'max_rel_diff_vs_fp64_cumsum': maxrel}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--config', choices=CONFIGS, help='run one configuration in this process (child mode)')
  ap.add_argument('--small', action='store_true', help='toy sizes (a rehearsal of the script, not a measurement)')
  ap.add_argument('--timeout', type=int, default=240, help='seconds per configuration')
  ap.add_argument('--out', help='also write the JSON line to this file')
  args = ap.parse_args()
  if args.config:
    print('SCAN_BENCH ' + json.dumps(run_config(args.config, args.small)), flush=True)
    return 0
  results, failed = [], None
  for name in CONFIGS:
    cmd = ['timeout', '-k', '10', str(args.timeout), sys.executable, os.path.abspath(__file__), '--config', name]
    if args.small:
      cmd.append('--small')
    r = subprocess.run(cmd, capture_output=True, text=True)
    line = [l for l in r.stdout.splitlines() if l.startswith('SCAN_BENCH ')]
    if r.returncode != 0 or not line:
      failed = {'config': name, 'exit': r.returncode, 'stderr': r.stderr[-2000:]}
      break  # nothing more is started on the GPU after a failure
    results.append(json.loads(line[-1][len('SCAN_BENCH '):]))
  doc = {'tool': 'scan_bench', 'dtype': 'float32', 'warmup': WARMUP, 'steps': STEPS, 'small': bool(args.small),
         'bytes_model': '2*N*4', 'configs': results}
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
