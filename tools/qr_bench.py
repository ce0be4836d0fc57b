"""Measure spx_geqr / spx_orgqr on one GPU.

Legs, both dtypes, Gaussian data of (2^20 x 16), (2^20 x 64) and (2^22 x 64):

  spx          geqr + orgqr (R and the explicit Q), and each alone.

Beside each leg, from the same run:

  scipy        scipy.linalg.qr(mode='economic') on this box's CPU -- the only
               route a user of the parent commit, which has no qr, had;
  choleskyqr   the reference's algorithm (spartan/examples/ssvd/qr.py) from this
               project's own kernels: A^T A (spx_gemm, the transposed copy made
               outside the timed region), its Cholesky factor (spx_potrf) and
               Q = A R^-1 (spx_trsm RIGHT / T on a copy of A);
  torch        torch.linalg.qr(mode='reduced') on the GPU, if the installed
               torch provides it (otherwise the JSON says why not; a call that
               takes more than --slow-ms is timed once, not every round).

GPU legs are timed with HIP events after warm-up, in interleaved rounds in one
process (round r runs every leg once), and report the median and the minimum.
Every GPU row also reports ``traffic_fraction``: the time to move 4 m n
elements (A read, reflectors written and read, Q written) at 8 TB/s over the
row's median time.  Before anything is timed each factorization is checked on
the GPU in float64 (``check`` in the JSON: the normwise residual and
||Q^T Q - I||_F, the Gram matrix summed at two levels, for spx, choleskyqr and
torch).  Nothing here asserts a speed.

Prints one JSON line and writes it to --out.

  python tools/qr_bench.py --out profiles/qr_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12
SHAPES = ((2 ** 20, 16), (2 ** 20, 64), (2 ** 22, 64))


def _summary(ms, ideal_ms):
  med, mn = statistics.median(ms), min(ms)
  return {'ms_median': round(med, 4), 'ms_min': round(mn, 4), 'traffic_fraction': round(ideal_ms / med, 4),
          'runs': len(ms)}


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'qr_bench.json'))
  ap.add_argument('--rounds', type=int, default=5)
  ap.add_argument('--warmup', type=int, default=2)
  ap.add_argument('--cpu-runs', type=int, default=1)
  ap.add_argument('--slow-ms', type=float, default=1500.0)
  ap.add_argument('--shapes', type=str, nargs='*', default=['%dx%d' % s for s in SHAPES])
  args = ap.parse_args()
  import numpy as np
  import scipy.linalg
  import torch
  import spartan_amd
  from spartan_amd import backend
  spartan_amd.initialize()
  be = backend.get()
  dev = torch.device('cuda', torch.cuda.current_device())
  shapes = [tuple(int(v) for v in s.split('x')) for s in args.shapes]
  res = {'device': torch.cuda.get_device_name(dev), 'rounds': args.rounds, 'warmup': args.warmup,
         'hbm_bytes_per_s': HBM_BYTES_PER_S, 'qr': {}, 'plan': {}, 'check': {}}
  legs = []  # (key, which, fn, ideal_ms)
  fro = torch.linalg.matrix_norm

  def gram(q, chunk=1024):
    # Q^T Q summed at two levels (chunks of rows, then the chunks' sums): one float64 product over all m rows
    # carries a summation error that grows as sqrt(m) u and hides a float64 factor's own few u
    m, n = q.shape
    q = q.contiguous()
    k = m // chunk
    g = torch.zeros((n, n), dtype=q.dtype, device=q.device)
    if k:
      blocks = q[:k * chunk].view(k, chunk, n)
      g += torch.bmm(blocks.transpose(1, 2), blocks).sum(0)
    if m > k * chunk:
      g += q[k * chunk:].t() @ q[k * chunk:]
    return g

  def check(A, Q, R):
    a, q, r = A.double(), Q.double(), R.double()
    n = A.shape[1]
    return {'residual': float((fro(a - q @ r) / fro(a)).item()),
            'orthogonality': float(fro(gram(q) - torch.eye(n, dtype=torch.float64, device=dev)).item())}

  for dtype in ('float32', 'float64'):
    tdt = getattr(torch, dtype)
    es = 4 if dtype == 'float32' else 8
    for m, n in shapes:
      key = '%s_%dx%d' % (dtype, m, n)
      nmax, r = backend.geqr_plan(np.dtype(dtype), n)
      res['plan'][key] = {'nmax': nmax, 'r': r,
                          'workspace_bytes': int(be.lib.spx_geqr_workspace(backend.spx_dtype(np.dtype(dtype)), m, n))}
      ideal = 4.0 * m * n * es / HBM_BYTES_PER_S * 1e3
      A = torch.randn((m, n), dtype=tdt, device=dev)
      Q = torch.empty_like(A)
      R, h = be.geqr(A)
      be.orgqr(h, None, Q)
      res['check'][key] = {'spx': check(A, Q, R)}
      row = res['qr'].setdefault(key, {'ideal_ms': round(ideal, 4)})

      def spx(A=A, Q=Q):
        _R, hh = be.geqr(A)
        be.orgqr(hh, None, Q)
      legs.append((key, 'spx', spx, ideal))
      legs.append((key, 'spx_geqr', (lambda A=A: be.geqr(A)), ideal))
      legs.append((key, 'spx_orgqr', (lambda h=h, Q=Q: be.orgqr(h, None, Q)), ideal))

      # the reference's CholeskyQR on this project's kernels
      At = A.t().contiguous()
      G = torch.empty((n, n), dtype=tdt, device=dev)
      L = torch.empty_like(G)
      Qc = torch.empty_like(A)

      def choleskyqr(A=A, At=At, G=G, L=L, Qc=Qc):
        be.gemm(At, A, G)
        info = be.potrf(G, L)
        Qc.copy_(A)
        be.trsm(L, Qc, side='R', trans=True)
        return info
      try:
        info = choleskyqr()
        if int(info.item()) != 0:
          raise RuntimeError('spx_potrf info = %d' % int(info.item()))
        res['check'][key]['choleskyqr'] = check(A, Qc, L.t())
        legs.append((key, 'choleskyqr', choleskyqr, ideal))
      except Exception as e:
        row['choleskyqr'] = {'unavailable': '%s: %s' % (type(e).__name__, str(e)[:200])}

      def tqr(A=A):
        return torch.linalg.qr(A, mode='reduced')
      try:
        tqr()  # first call: library set-up
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tq, tr = tqr()
        torch.cuda.synchronize()
        once = (time.perf_counter() - t0) * 1e3
        res['check'][key]['torch'] = check(A, tq, tr)
        del tq, tr
        if once > args.slow_ms:
          row['torch'] = dict(_summary([once], ideal), timed='one host-timed call (slower than --slow-ms)')
        else:
          legs.append((key, 'torch', tqr, ideal))
      except Exception as e:  # the installed torch has no such solver
        row['torch'] = {'unavailable': '%s: %s' % (type(e).__name__, str(e)[:200])}
      Ah = A.cpu().numpy()
      ts = []
      for _ in range(args.cpu_runs):
        t0 = time.perf_counter()
        scipy.linalg.qr(Ah, mode='economic', check_finite=False)
        ts.append((time.perf_counter() - t0) * 1e3)
      row['scipy_cpu'] = dict(_summary(ts, ideal), cpus=len(os.sched_getaffinity(0)))
      del Ah
      sys.stderr.write('qr_bench: %s set up\n' % key)
  times = {i: [] for i in range(len(legs))}
  for r in range(args.warmup + args.rounds):
    sys.stderr.write('qr_bench: round %d of %d\n' % (r + 1, args.warmup + args.rounds))
    for i, leg in enumerate(legs):
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      leg[2]()
      b.record()
      b.synchronize()
      if r >= args.warmup:
        times[i].append(a.elapsed_time(b))
  for i, (key, which, _fn, ideal) in enumerate(legs):
    res['qr'][key][which] = _summary(times[i], ideal)
  line = json.dumps(res, sort_keys=True)
  print(line)
  with open(args.out, 'w') as f:
    f.write(line + '\n')


if __name__ == '__main__':
  main()
