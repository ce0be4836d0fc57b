"""Measure spx_als_solve on one GPU.

A synthetic rating matrix of 2^18 users x 2^14 items with 64 ratings per user
(2^24 stored entries, columns uniform at random, values in [1, 5]), solved on
the user side (rows of A: 64 entries each) and on the item side (rows of A^T,
made on the host by scipy: about 1024 entries each), for f = 20 and f = 64,
float32 and float64.  Each leg is timed by HIP events around single calls after
warm-up; median and minimum over the rounds.  ``fraction`` is the time to move
the bytes of the model

    nnz f itemsize  (the gathered factor rows)  +  m f itemsize  (X)
      +  nnz (4 + itemsize) + 8 (m + 1)  (the CSR arrays)

at 8 TB/s over the median time.  There is no other implementation beside it:
the byte model is the only yardstick.  Before a leg is timed, 64 of its rows
are compared with a float64 NumPy solve (the largest relative error is
printed).  Nothing here asserts a speed.

  python tools/als_bench.py --out profiles/als_bench.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8e12


def _events(fn, torch):
  a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  a.record()
  fn()
  b.record()
  b.synchronize()
  return a.elapsed_time(b)


def _check_rows(np, A, Y, lam, X, rows):
  worst = 0.0
  for i in rows:
    a, b = A.indptr[i], A.indptr[i + 1]
    Yi = Y[A.indices[a:b]].astype(np.float64)
    G = Yi.T.dot(Yi) + lam * (b - a) * np.eye(Y.shape[1])
    x = np.linalg.solve(G, Yi.T.dot(A.data[a:b].astype(np.float64))) if b > a else np.zeros(Y.shape[1])
    worst = max(worst, float(np.abs(X[i] - x).max() / max(np.abs(x).max(), 1e-300)))
  return worst


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'als_bench.txt'))
  ap.add_argument('--log2-users', type=int, default=18)
  ap.add_argument('--log2-items', type=int, default=14)
  ap.add_argument('--per-user', type=int, default=64)
  ap.add_argument('--rounds', type=int, default=10)
  ap.add_argument('--warmup', type=int, default=3)
  ap.add_argument('--features', type=int, nargs='*', default=[20, 64])
  args = ap.parse_args()
  import numpy as np
  import scipy.sparse as sp
  m, n, L = 1 << args.log2_users, 1 << args.log2_items, args.per_user
  rs = np.random.RandomState(0)
  cols = np.sort(rs.randint(0, n, (m, L)), axis=1).astype(np.int32)
  vals = rs.randint(1, 6, (m, L)).astype(np.float64)
  indptr = np.arange(m + 1, dtype=np.int64) * L
  users = sp.csr_matrix((vals.reshape(-1), cols.reshape(-1), indptr), shape=(m, n))
  items = users.T.tocsr()  # duplicates of a (user, item) pair stay separate entries on both sides
  items.sort_indices()
  lam = 0.065

  import torch
  if not torch.cuda.is_available():
    sys.exit('als_bench: no GPU')
  from spartan_amd import backend
  be = backend.HipBackend()
  lines = ['spx_als_solve, %d users x %d items, %d stored entries, lambda %g; HIP events per call, median / minimum of %d '
           'after %d warm-up calls; fraction: the byte model at 8 TB/s over the median' % (m, n, users.nnz, lam,
                                                                                        args.rounds, args.warmup)]
  for dtype in (np.float32, np.float64):
    es = np.dtype(dtype).itemsize
    for f in args.features:
      for side, A in (('users', users), ('items', items)):
        rows, other = A.shape
        Y = (0.5 + rs.random_sample((other, f))).astype(dtype)
        dev = [torch.as_tensor(a).cuda() for a in (A.indptr.astype(np.int64), A.indices.astype(np.int32),
                                                   A.data.astype(dtype), Y)]
        X = torch.empty((rows, f), dtype=backend.torch_dtype(dtype), device='cuda')

        def call():
          return be.als_solve(dev[0], dev[1], dev[2], other, dev[3], lam, X)

        info = int(call().item())
        err = _check_rows(np, A, Y, lam, X.cpu().numpy(), rs.choice(rows, 64, replace=False))
        for _ in range(args.warmup):
          call()
        ts = [_events(call, torch) for _ in range(args.rounds)]
        med = statistics.median(ts)
        nbytes = A.nnz * f * es + rows * f * es + A.nnz * (4 + es) + 8 * (rows + 1)
        lines.append('%-7s f=%-2d %-5s rows %7d longest row %6d  median %9.3f ms  min %9.3f ms  model %7.1f MB  '
                     'fraction %.4f  failed rows %d  rel err of 64 rows %.2e'
                     % (np.dtype(dtype).name, f, side, rows, int(np.diff(A.indptr).max()), med, min(ts), nbytes / 1e6,
                        nbytes / HBM_BYTES_PER_S / (med * 1e-3), info, err))
        print(lines[-1], flush=True)
  os.makedirs(os.path.dirname(args.out), exist_ok=True)
  with open(args.out, 'w') as fh:
    fh.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
  main()
