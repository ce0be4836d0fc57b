"""Measure spx_gesvj and the tall route of ``expr.svd`` on one GPU.

Legs, both dtypes, Gaussian data:

  direct  square n in {16, 64, nmax} x batch in {1, 256, 4096}:
          HipBackend.gesvj (U, S and Vt of the whole batch in one launch);
  tall    (2^20, 64) and (2^20, nmax_qr) in one tile: ``expr.svd`` forced (the
          TSQR, gesvj of R, U = Q U_R, the info read).

Beside each leg, from the same run:

  host    the only route a user of the parent commit, which has no svd, had:
          the data copied to the host, ``scipy.linalg.svd`` per matrix on this
          box's CPU threads, the factors copied back (wall clock, the copies
          included);
  torch   ``torch.linalg.svd(full_matrices=False)`` of the installed torch on
          the same GPU, if it provides one (otherwise the JSON says why not; a
          first call that takes more than --slow-ms is the one timing, on the
          host clock, and the leg does not join the rounds).

GPU legs are timed with HIP events after warm-up, in interleaved rounds in one
process (round r runs every leg once), and report the median and the minimum.
Every spx row also carries the sweep counts the kernel reported (min / max
over the batch) and, before anything is timed, a check in float64 on the GPU
(``check`` in the JSON: the largest normwise residual ||A - U diag(s) Vt||_F /
||A||_F, ||U^T U - I||_F and ||Vt Vt^T - I||_F over the batch, for spx and
torch).  Host and torch legs that would start after --budget-s seconds are
skipped and say so.  Nothing here asserts a speed.

Prints one JSON line and writes it to --out.

  python tools/svd_bench.py --out profiles/svd_bench.json
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
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'svd_bench.json'))
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--warmup', type=int, default=2)
  ap.add_argument('--slow-ms', type=float, default=500.0)
  ap.add_argument('--budget-s', type=float, default=420.0)
  ap.add_argument('--batches', type=int, nargs='*', default=list(BATCHES))
  ap.add_argument('--tall-rows', type=int, default=1 << 20)
  args = ap.parse_args()
  import numpy as np
  import scipy.linalg
  import torch
  import spartan_amd
  from spartan_amd import backend, expr
  from spartan_amd.array import distarray, extent
  from spartan_amd.expr.base import eval_cache
  spartan_amd.initialize()
  be = backend.get()
  dev = torch.device('cuda', torch.cuda.current_device())
  start = time.perf_counter()
  res = {'device': torch.cuda.get_device_name(dev), 'rounds': args.rounds, 'warmup': args.warmup,
         'cpus': len(os.sched_getaffinity(0)), 'svd': {}, 'plan': {}, 'check': {}}
  legs = []  # (key, which, fn)
  fro = torch.linalg.matrix_norm

  def late():
    return time.perf_counter() - start > args.budget_s

  def check(A, U, s, Vt):
    a, u, sd, vt = A.double(), U.double(), s.double(), Vt.double()
    eye = torch.eye(A.shape[-1], dtype=torch.float64, device=dev)
    return {'residual': float((fro(a - (u * sd[..., None, :]) @ vt) / fro(a)).max().item()),
            'orthogonality_u': float(fro(u.transpose(-1, -2) @ u - eye).max().item()),
            'orthogonality_vt': float(fro(vt @ vt.transpose(-1, -2) - eye).max().item())}

  def beside(key, row, A):
    """The torch and host legs of the device tensor ``A`` ((B, m, n) or (m, n))."""
    def tsvd(A=A):
      return torch.linalg.svd(A, full_matrices=False)
    if late():
      row['torch'] = {'skipped': 'past --budget-s'}
    else:
      try:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tu, ts, tv = tsvd()  # the first call (with the library's set-up: milliseconds)
        torch.cuda.synchronize()
        once = (time.perf_counter() - t0) * 1e3
        res['check'][key]['torch'] = check(A, tu, ts, tv)
        del tu, ts, tv
        if once > args.slow_ms:
          row['torch'] = dict(_summary([once]), timed='its first call, host-timed (slower than --slow-ms)')
        else:
          legs.append((key, 'torch', tsvd))
      except Exception as e:  # the installed torch has no such solver
        row['torch'] = {'unavailable': '%s: %s' % (type(e).__name__, str(e)[:200])}
    if late():
      row['host_scipy'] = {'skipped': 'past --budget-s'}
      return
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    Ah = A.cpu().numpy()
    stack = Ah.reshape((-1,) + Ah.shape[-2:])
    out = [scipy.linalg.svd(x, full_matrices=False, check_finite=False) for x in stack]
    back = [torch.as_tensor(np.stack([o[i] for o in out])).to(dev) for i in range(3)]
    torch.cuda.synchronize()
    row['host_scipy'] = _summary([(time.perf_counter() - t0) * 1e3])
    del Ah, stack, out, back

  for dtype in ('float32', 'float64'):
    tdt = getattr(torch, dtype)
    nmax, _, sweep_max = backend.gesvj_plan(np.dtype(dtype), 1)
    nq = min(backend.geqr_plan(np.dtype(dtype), 1)[0], nmax)
    res['plan'][dtype] = {'nmax': nmax, 'sweep_max': sweep_max, 'nmax_qr': nq,
                          'mmax': {str(n): backend.gesvj_plan(np.dtype(dtype), n)[1] for n in (16, 64, nmax)}}
    for n in (16, 64, nmax):
      for batch in args.batches:
        key = '%s_n%d_b%d' % (dtype, n, batch)
        A = torch.randn((batch, n, n), dtype=tdt, device=dev)
        U, s, Vt, info = be.gesvj(A)
        ih = info.cpu().numpy()
        row = res['svd'].setdefault(key, {})
        row['sweeps'] = {'min': int(ih.min()), 'max': int(ih.max())}
        res['check'][key] = {'spx': check(A, U, s, Vt)}
        del U, s, Vt, info
        legs.append((key, 'spx', (lambda A=A: be.gesvj(A))))
        legs.append((key, 'spx_values_only', (lambda A=A: be.gesvj(A, compute_uv=False))))
        beside(key, row, A)
        sys.stderr.write('svd_bench: %s set up\n' % key)
  for dtype in ('float32', 'float64'):
    tdt = getattr(torch, dtype)
    m = args.tall_rows
    for n in sorted({64, res['plan'][dtype]['nmax_qr']}):
      key = '%s_tall_%dx%d' % (dtype, m, n)
      A = torch.randn((m, n), dtype=tdt, device=dev)
      full = extent.from_shape((m, n))
      arr = distarray.from_tiles((m, n), np.dtype(dtype), {full: 0}, {full: A})

      def tall(arr=arr):
        eval_cache.clear()
        return tuple(e.force() for e in expr.svd(expr.lazify(arr)))
      infos = []
      real = be.gesvj

      def spy(*a, **k):
        out = real(*a, **k)
        infos.append(out[3])
        return out
      be.gesvj = spy
      try:
        Ua, sa, Vta = tall()
      finally:
        del be.gesvj
      row = res['svd'].setdefault(key, {})
      ih = torch.cat(infos).cpu().numpy()
      row['sweeps'] = {'min': int(ih.min()), 'max': int(ih.max())}
      res['check'][key] = {'spx': check(A, Ua.fetch(full), sa.device_data(), Vta.device_data())}
      del Ua, sa, Vta
      legs.append((key, 'spx', tall))
      beside(key, row, A)
      sys.stderr.write('svd_bench: %s set up\n' % key)
  times = {i: [] for i in range(len(legs))}
  for r in range(args.warmup + args.rounds):
    sys.stderr.write('svd_bench: round %d of %d\n' % (r + 1, args.warmup + args.rounds))
    for i, leg in enumerate(legs):
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      leg[2]()
      b.record()
      b.synchronize()
      if r >= args.warmup:
        times[i].append(a.elapsed_time(b))
  for i, (key, which, _fn) in enumerate(legs):
    res['svd'][key][which] = _summary(times[i])
  for key, row in res['svd'].items():
    spx = row['spx']['ms_median']
    if 'ms_median' in row.get('host_scipy', {}):
      row['host_over_spx'] = round(row['host_scipy']['ms_median'] / spx, 3)
    if 'ms_median' in row.get('torch', {}):
      row['torch_over_spx'] = round(row['torch']['ms_median'] / spx, 3)
  res['seconds'] = round(time.perf_counter() - start, 1)
  line = json.dumps(res, sort_keys=True)
  print(line)
  with open(args.out, 'w') as f:
    f.write(line + '\n')


if __name__ == '__main__':
  main()
