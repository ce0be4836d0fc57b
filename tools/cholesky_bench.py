"""Measure spx_potrf / spx_trsm / spx_syrk on one GPU.

Legs, both dtypes, n = 6400 (the size of the reference's tests/test_cholesky.py
benchmark) and n = 16384:

  potrf   the lower factor of G G^T / n + I, out of place;
  trsm    L X = B (LEFT / N) with 64 right-hand sides.

Beside each leg, from the same run:

  scipy   scipy.linalg.cholesky(lower=True) / solve_triangular on this box's
          CPU -- what a user of the parent commit, which has no GPU path,
          would call;
  torch   torch.linalg.cholesky / torch.linalg.solve_triangular on the GPU, if
          the installed torch provides them (otherwise the JSON says why not).

GPU legs are timed with HIP events after warm-up, in interleaved rounds in one
process (round r runs every leg once), and report the median and the minimum;
the CPU legs run ``--cpu-runs`` times each.  potrf rows report TF/s over n^3 / 3
flops, trsm rows over n^2 nrhs, and that as a fraction of the dtype's dense
MFMA peak (the figures bench.py uses for dot).

Separately: the update kernel (C -= A B^T, plain and ``lower``) on M = N = 8192
at K = nb and K = nb_outer beside the project's own spx_gemm on the same M, N,
K -- whether one panel level would do is read off these rows.

Before anything is timed each factor and solution is checked on the GPU
against the normwise form of the error contract (``check`` in the JSON).

Prints one JSON line and writes it to --out.

  python tools/cholesky_bench.py --out profiles/cholesky_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MFMA_PEAK_TFS = {'float32': 157.3, 'float64': 78.6}  # bench.py: MFMA_F32_TFS, MFMA_F64_TFS
SIZES = (6400, 16384)
NRHS = 64
UPD = 8192


def _summary(ms, flops, dtype):
  med, mn = statistics.median(ms), min(ms)
  return {'ms_median': round(med, 4), 'ms_min': round(mn, 4), 'tfs_median': round(flops / med / 1e9, 3),
          'tfs_min_time': round(flops / mn / 1e9, 3),
          'peak_fraction': round(flops / med / 1e9 / MFMA_PEAK_TFS[dtype], 4), 'runs': len(ms)}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'cholesky_bench.json'))
  ap.add_argument('--rounds', type=int, default=7)
  ap.add_argument('--warmup', type=int, default=2)
  ap.add_argument('--cpu-runs', type=int, default=2)
  ap.add_argument('--sizes', type=int, nargs='*', default=list(SIZES))
  args = ap.parse_args()
  import numpy as np
  import scipy.linalg
  import torch
  import spartan_amd
  from spartan_amd import backend
  spartan_amd.initialize()
  be = backend.get()
  dev = torch.device('cuda', torch.cuda.current_device())
  res = {'device': torch.cuda.get_device_name(dev), 'rounds': args.rounds, 'warmup': args.warmup, 'nrhs': NRHS,
         'mfma_peak_tfs': MFMA_PEAK_TFS, 'potrf': {}, 'trsm': {}, 'update': {}, 'plan': {}, 'check': {}}
  legs = []  # (section, key, which, fn, flops, dtype)
  keep = []
  for dtype in ('float32', 'float64'):
    tdt = getattr(torch, dtype)
    nb, nbo = backend.potrf_plan(np.dtype(dtype))
    res['plan'][dtype] = {'nb': nb, 'nb_outer': nbo}
    for n in args.sizes:
      G = torch.randn((n, n), dtype=tdt, device=dev)
      A = torch.matmul(G, G.t()) / n + torch.eye(n, dtype=tdt, device=dev)
      del G
      L = torch.empty_like(A)
      info = be.potrf(A, L)
      assert int(info.item()) == 0
      B0 = torch.randn((n, NRHS), dtype=tdt, device=dev)
      X = B0.clone()
      be.trsm(L, X, side='L', trans=False)
      keep.append((A, L, B0, X))
      key = '%s_n%d' % (dtype, n)
      # checked before anything is timed: the Frobenius forms of the entrywise bounds of DESIGN 3.18
      # (|| |L| |L|^T ||_F <= tr(A) <= sqrt(n) ||A||_F; || |L| |X| ||_F <= ||L||_F ||X||_F), doubled for the
      # check's own matmul
      u = 2.0 ** -24 if dtype == 'float32' else 2.0 ** -53
      fro = torch.linalg.matrix_norm
      r_f = float((fro(A - torch.matmul(L, L.t())) / fro(A)).item())
      r_s = float((fro(torch.matmul(L, X) - B0) / (fro(L) * fro(X))).item())
      res['check'][key] = {'potrf_residual': r_f, 'potrf_bound': 2 * (n + 1) * u * n ** 0.5,
                           'trsm_residual': r_s, 'trsm_bound': 2 * n * u}
      assert r_f <= res['check'][key]['potrf_bound'] and r_s <= res['check'][key]['trsm_bound'], res['check'][key]
      sys.stderr.write('cholesky_bench: %s set up\n' % key)
      legs.append(('potrf', key, 'spx', (lambda A=A, W=torch.empty_like(A): be.potrf(A, W)), n ** 3 / 3.0, dtype))

      def trsm(L=L, B0=B0, X=X):
        X.copy_(B0)
        be.trsm(L, X, side='L', trans=False)
      legs.append(('trsm', key, 'spx', trsm, float(n) * n * NRHS, dtype))
      for sec, name, fn in (('potrf', 'cholesky', lambda A=A: torch.linalg.cholesky(A)),
                            ('trsm', 'solve_triangular',
                             lambda L=L, B0=B0: torch.linalg.solve_triangular(L, B0, upper=False))):
        try:
          fn()
          torch.cuda.synchronize()
          legs.append((sec, key, 'torch', fn, n ** 3 / 3.0 if sec == 'potrf' else float(n) * n * NRHS, dtype))
        except Exception as e:  # the installed torch has no such solver
          res[sec].setdefault(key, {})['torch'] = {'unavailable': '%s: %s' % (type(e).__name__, str(e)[:200])}
      # the CPU legs, on the same matrices
      Ah, Bh = A.cpu().numpy(), B0.cpu().numpy()
      Lh = None
      for sec in ('potrf', 'trsm'):
        ts = []
        for _ in range(args.cpu_runs):
          t0 = time.perf_counter()
          if sec == 'potrf':
            Lh = scipy.linalg.cholesky(Ah, lower=True, check_finite=False)
          else:
            scipy.linalg.solve_triangular(Lh, Bh, lower=True, check_finite=False)
          ts.append((time.perf_counter() - t0) * 1e3)
        flops = n ** 3 / 3.0 if sec == 'potrf' else float(n) * n * NRHS
        res[sec].setdefault(key, {})['scipy_cpu'] = dict(_summary(ts, flops, dtype), cpus=len(os.sched_getaffinity(0)))
      del Ah, Bh, Lh
    # the update kernel against spx_gemm at the same shape
    for K in (nb, nbo):
      Ap = torch.randn((UPD, K), dtype=tdt, device=dev)
      Bp = torch.randn((UPD, K), dtype=tdt, device=dev)
      Bt = Bp.t().contiguous()
      C = torch.zeros((UPD, UPD), dtype=tdt, device=dev)
      key = '%s_K%d' % (dtype, K)
      fl = 2.0 * UPD * UPD * K
      legs.append(('update', key, 'spx_syrk', (lambda Ap=Ap, Bp=Bp, C=C: be.syrk(Ap, Bp, C)), fl, dtype))
      legs.append(('update', key, 'spx_syrk_lower', (lambda Ap=Ap, C=C: be.syrk(Ap, Ap, C, lower=True)), fl / 2, dtype))
      legs.append(('update', key, 'spx_gemm', (lambda Ap=Ap, Bt=Bt, C=C: be.gemm(Ap, Bt, C)), fl, dtype))
      keep.append((Ap, Bp, Bt, C))
  times = {i: [] for i in range(len(legs))}
  for r in range(args.warmup + args.rounds):
    sys.stderr.write('cholesky_bench: round %d of %d\n' % (r + 1, args.warmup + args.rounds))
    for i, leg in enumerate(legs):
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      leg[3]()
      b.record()
      b.synchronize()
      if r >= args.warmup:
        times[i].append(a.elapsed_time(b))
  for i, (sec, key, which, _fn, flops, dtype) in enumerate(legs):
    res[sec].setdefault(key, {})[which] = _summary(times[i], flops, dtype)
  line = json.dumps(res, sort_keys=True)
  print(line)
  with open(args.out, 'w') as f:
    f.write(line + '\n')


if __name__ == '__main__':
  main()
