"""Measure spx_syevj on one GPU.

Legs, both dtypes, symmetrised Gaussian data: n in {16, 64, nmax} x batch in
{1, 256, 4096}.

  spx     HipBackend.syevj (eigenvalues and eigenvectors of the whole batch in
          one launch).

Beside each leg, from the same run:

  host    the only route a user of the parent commit, which has no eigh, had:
          the batch copied to the host, ``scipy.linalg.eigh(driver='evd')`` per
          matrix on this box's CPU threads, w and V copied back (wall clock,
          the copies included);
  torch   ``torch.linalg.eigh`` of the installed torch on the same GPU, if it
          provides one (otherwise the JSON says why not; a call that takes more
          than --slow-ms is timed once, not every round).

GPU legs are timed with HIP events after warm-up, in interleaved rounds in one
process (round r runs every leg once), and report the median and the minimum.
Every spx row also carries the sweep counts the kernel reported (min / max
over the batch) and, before anything is timed, a check in float64 on the GPU
(``check`` in the JSON: the largest normwise residual ||A V - V diag(w)||_F /
||A||_F and ||V^T V - I||_F over the batch, for spx and torch).  Nothing here
asserts a speed.

Prints one JSON line and writes it to --out.

  python tools/eigh_bench.py --out profiles/eigh_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BATCHES = (1, 256, 4096)


def _summary(ms):
  return {'ms_median': round(statistics.median(ms), 4), 'ms_min': round(min(ms), 4), 'runs': len(ms)}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'eigh_bench.json'))
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--warmup', type=int, default=2)
  ap.add_argument('--cpu-runs', type=int, default=1)
  ap.add_argument('--slow-ms', type=float, default=500.0)
  ap.add_argument('--batches', type=int, nargs='*', default=list(BATCHES))
  args = ap.parse_args()
  import numpy as np
  import scipy.linalg
  import torch
  import spartan_amd
  from spartan_amd import backend
  spartan_amd.initialize()
  be = backend.get()
  dev = torch.device('cuda', torch.cuda.current_device())
  res = {'device': torch.cuda.get_device_name(dev), 'rounds': args.rounds, 'warmup': args.warmup,
         'cpus': len(os.sched_getaffinity(0)), 'eigh': {}, 'plan': {}, 'check': {}}
  legs = []  # (key, which, fn)
  fro = torch.linalg.matrix_norm

  def check(A, w, V):
    a, wd, v = A.double(), w.double(), V.double()
    eye = torch.eye(A.shape[-1], dtype=torch.float64, device=dev)
    return {'residual': float((fro(a @ v - v * wd[:, None, :]) / fro(a)).max().item()),
            'orthogonality': float(fro(v.transpose(1, 2) @ v - eye).max().item())}

  for dtype in ('float32', 'float64'):
    tdt = getattr(torch, dtype)
    nmax, sweep_max = backend.syevj_plan(np.dtype(dtype))
    res['plan'][dtype] = {'nmax': nmax, 'sweep_max': sweep_max}
    for n in (16, 64, nmax):
      for batch in args.batches:
        key = '%s_n%d_b%d' % (dtype, n, batch)
        G = torch.randn((batch, n, n), dtype=tdt, device=dev)
        A = ((G + G.transpose(1, 2)) / 2).contiguous()
        del G
        w, V, info = be.syevj(A)
        ih = info.cpu().numpy()
        row = res['eigh'].setdefault(key, {})
        row['sweeps'] = {'min': int(ih.min()), 'max': int(ih.max())}
        res['check'][key] = {'spx': check(A, w, V)}
        del w, V, info
        legs.append((key, 'spx', (lambda A=A: be.syevj(A))))

        def teigh(A=A):
          return torch.linalg.eigh(A)
        try:
          teigh()  # first call: library set-up
          torch.cuda.synchronize()
          t0 = time.perf_counter()
          tw, tv = teigh()
          torch.cuda.synchronize()
          once = (time.perf_counter() - t0) * 1e3
          res['check'][key]['torch'] = check(A, tw, tv)
          del tw, tv
          if once > args.slow_ms:
            row['torch'] = dict(_summary([once]), timed='one host-timed call (slower than --slow-ms)')
          else:
            legs.append((key, 'torch', teigh))
        except Exception as e:  # the installed torch has no such solver
          row['torch'] = {'unavailable': '%s: %s' % (type(e).__name__, str(e)[:200])}

        ts = []
        for _ in range(args.cpu_runs):
          torch.cuda.synchronize()
          t0 = time.perf_counter()
          Ah = A.cpu().numpy()
          wh, vh = np.empty((batch, n), Ah.dtype), np.empty_like(Ah)
          for b in range(batch):
            wh[b], vh[b] = scipy.linalg.eigh(Ah[b], driver='evd', check_finite=False)
          wd, vd = torch.as_tensor(wh).to(dev), torch.as_tensor(vh).to(dev)
          torch.cuda.synchronize()
          ts.append((time.perf_counter() - t0) * 1e3)
          del Ah, wh, vh, wd, vd
        row['host_scipy'] = _summary(ts)
        sys.stderr.write('eigh_bench: %s set up\n' % key)
  times = {i: [] for i in range(len(legs))}
  for r in range(args.warmup + args.rounds):
    sys.stderr.write('eigh_bench: round %d of %d\n' % (r + 1, args.warmup + args.rounds))
    for i, leg in enumerate(legs):
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      leg[2]()
      b.record()
      b.synchronize()
      if r >= args.warmup:
        times[i].append(a.elapsed_time(b))
  for i, (key, which, _fn) in enumerate(legs):
    res['eigh'][key][which] = _summary(times[i])
  for key, row in res['eigh'].items():
    spx = row['spx']['ms_median']
    row['host_over_spx'] = round(row['host_scipy']['ms_median'] / spx, 3)
    if 'ms_median' in row.get('torch', {}):
      row['torch_over_spx'] = round(row['torch']['ms_median'] / spx, 3)
  line = json.dumps(res, sort_keys=True)
  print(line)
  with open(args.out, 'w') as f:
    f.write(line + '\n')


if __name__ == '__main__':
  main()
