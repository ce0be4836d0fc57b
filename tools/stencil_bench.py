"""Measure ``stencil`` / ``maxpool`` (spx_stencil, spx_maxpool) on the
reference's convnet benchmark (tests/benchmark_convnet.py there) on one GPU.

Workload: images (64, 3, 256, 256), 64 filters of 4 x 4, three layers of
``stencil`` followed by ``maxpool(2, 2)`` -- layers 2 and 3 see 64 channels at
128^2 and 64^2 -- in float64 (the reference's default) and float32.

Rows: conv1 pool1 conv2 pool2 conv3 pool3 and the whole chain.  Each is timed
with HIP events over 20 steps after 5 warm-up steps of the forced expression
(the expression layer's host work and the allocation of the result are inside
the timing).  Beside each row, from the same run on the same device tensors:

  torch   F.conv2d(F.pad(x, (0, fh - 1, 0, fw - 1)), w) and
          F.max_pool2d(F.pad(x, (0, p - 1, 0, p - 1), value=-inf), p, s),
          which equal the contract (ceil_mode=True does not when pool > stride
          or a side is shorter than the pool);
  gemm    the project's own spx_gemm on random matrices of the equivalent
          M = F, N = 64 W H, K = C fw fh (conv rows).

Conv rows report TF/s over the nominal 2 N F W H K and that as a fraction of
the dense MFMA peak bench.py uses for dot; pool rows TB/s over the input read
plus the output written.  Before anything is printed the results are checked
against torch's: conv within tol * (the same convolution of the absolute
values), tol 1e-5 (float32) / 1e-12 (float64); pool bit for bit.

Every dtype runs in a child process of its own under ``timeout -k 10``; after
a failed child nothing more is started.  Prints one JSON line (and writes it
to --out).

  python tools/stencil_bench.py --out profiles/stencil_bench_<tag>.json
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DTYPES = ['float64', 'float32']
WARMUP, STEPS = 5, 20
MFMA_PEAK_TFS = {'float32': 157.3, 'float64': 78.6}  # bench.py: MFMA_F32_TFS, MFMA_F64_TFS
TOL = {'float32': 1e-5, 'float64': 1e-12}


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
  return {'ms_min': round(ms[0], 4), 'ms': round(sum(ms) / len(ms), 4), 'ms_max': round(ms[-1], 4)}


def run_dtype(name, small):
  import numpy as np
  import torch
  import torch.nn.functional as F
  import spartan_amd
  from spartan_amd import backend, expr
  from spartan_amd.array import distarray
  from spartan_amd.expr import stencil
  spartan_amd.initialize()
  be = backend.get()
  assert isinstance(be, backend.HipBackend)
  dt = np.dtype(name)
  n_img, colors, size, n_filt, fs, pool = (4, 3, 32, 8, 4, 2) if small else (64, 3, 256, 64, 4, 2)
  tol = TOL[name]

  def tensor(val):  # the forced result as its one device tensor (one worker: one tile)
    (ex, tile), = val.local.items()
    return tile.data

  def one_tile(dev):  # a device tensor as a lazy one-tile array
    e = distarray.ext.from_shape(tuple(dev.shape))
    return expr.lazify(distarray.from_tiles(tuple(dev.shape), backend.np_dtype(dev.dtype), {e: 0}, {e: dev}))

  x = tensor(expr.rand(n_img, colors, size, size, dtype=dt, seed=17, low=-1.0, high=1.0).force())
  ws = [tensor(expr.rand(n_filt, c, fs, fs, dtype=dt, seed=20 + l, low=-1.0, high=1.0).force())
        for l, c in enumerate((colors, n_filt, n_filt))]
  t_conv = lambda t, w: F.conv2d(F.pad(t, (0, w.shape[3] - 1, 0, w.shape[2] - 1)), w)
  t_pool = lambda t: F.max_pool2d(F.pad(t, (0, pool - 1, 0, pool - 1), value=float('-inf')), pool, pool)
  rows = []

  def check(ok, what):  # a wrong result ends the child before anything is timed or printed
    if not ok:
      raise SystemExit('stencil_bench: %s %s does not match torch' % (name, what))
  cur = x
  for l, w in enumerate(ws):
    X, Wx = one_tile(cur), one_tile(w)
    n, c, W, H = cur.shape
    K = c * fs * fs
    ours = lambda: stencil.stencil(X, Wx, 2).force()
    got, want = tensor(ours()), t_conv(cur, w)
    mag = t_conv(cur.abs(), w.abs())
    ratio = float(((got - want).abs() / mag.clamp_min(1e-300)).max().item())
    check(got.shape == want.shape and ratio <= tol, 'conv%d (max |err| / mag %.3g, tol %g)' % (l + 1, ratio, tol))
    del want, mag
    flops = 2.0 * n * n_filt * W * H * K
    row = {'row': 'conv%d' % (l + 1), 'images': list(cur.shape), 'filters': list(w.shape), 'K': K,
           'max_err_over_mag_vs_torch': ratio, 'ours': _time(ours), 'torch': _time(lambda: t_conv(cur, w))}
    A = torch.rand((n_filt, K), dtype=cur.dtype, device=cur.device)
    Bm = torch.rand((K, n * W * H), dtype=cur.dtype, device=cur.device)
    C = torch.empty((n_filt, n * W * H), dtype=cur.dtype, device=cur.device)
    row['gemm'] = _time(lambda: be.gemm(A, Bm, C))
    row['gemm']['M_N_K'] = [n_filt, n * W * H, K]
    del A, Bm, C
    for k in ('ours', 'torch', 'gemm'):
      tf = flops / (row[k]['ms'] / 1e3) / 1e12
      row[k].update(tf_per_s=round(tf, 2), mfma_frac=round(tf / MFMA_PEAK_TFS[name], 4))
    row['ours_over_torch'] = round(row['ours']['ms'] / row['torch']['ms'], 3)
    row['rate_over_gemm'] = round(row['ours']['tf_per_s'] / row['gemm']['tf_per_s'], 3)
    rows.append(row)
    conv = got
    Cx = one_tile(conv)
    ours = lambda: stencil.maxpool(Cx, pool, pool).force()
    got, want = tensor(ours()), t_pool(conv)
    check(got.shape == want.shape and torch.equal(got, want), 'pool%d' % (l + 1))
    del want
    nbytes = (conv.numel() + got.numel()) * conv.element_size()
    row = {'row': 'pool%d' % (l + 1), 'images': list(conv.shape), 'ours': _time(ours),
           'torch': _time(lambda: t_pool(conv)), 'algorithmic_bytes': nbytes}
    for k in ('ours', 'torch'):
      row[k]['tb_per_s'] = round(nbytes / (row[k]['ms'] / 1e3) / 1e12, 3)
    row['ours_over_torch'] = round(row['ours']['ms'] / row['torch']['ms'], 3)
    rows.append(row)
    cur = got
    del conv

  X, Ws = one_tile(x), [one_tile(w) for w in ws]

  def chain():
    e = X
    for Wx in Ws:
      e = stencil.maxpool(stencil.stencil(e, Wx, 2), pool, pool)
    return expr.force(e)

  def t_chain():
    t = x
    for w in ws:
      t = t_pool(t_conv(t, w))
    return t
  got = tensor(chain())
  check(torch.equal(got, cur), 'chain (against its own layers)')  # the chain repeats the layers bit for bit
  row = {'row': 'chain', 'ours': _time(chain), 'torch': _time(t_chain)}
  row['ours_over_torch'] = round(row['ours']['ms'] / row['torch']['ms'], 3)
  rows.append(row)
  return {'dtype': name, 'tile': list(backend.stencil_plan(dt)), 'rows': rows, 'equal_torch': True}


def table(doc):
  out = []
  for d in doc['dtypes']:
    out.append('%s (block tile %s)' % (d['dtype'], 'x'.join(str(v) for v in d['tile'])))
    out.append('  row     ours ms min-mean-max        rate          torch ms    gemm ms   ours/torch')
    for r in d['rows']:
      o, t = r['ours'], r['torch']
      rate = ('%6.1f TF/s %4.1f%%' % (o['tf_per_s'], 100 * o['mfma_frac']) if 'tf_per_s' in o
              else ('%6.2f TB/s      ' % o['tb_per_s'] if 'tb_per_s' in o else ' ' * 17))
      out.append('  %-6s %7.3f %7.3f %7.3f  %s  %9.3f  %9s   %6.3f'
                 % (r['row'], o['ms_min'], o['ms'], o['ms_max'], rate, t['ms'],
                    '%.3f' % r['gemm']['ms'] if 'gemm' in r else '-', r['ours_over_torch']))
  return '\n'.join(out)


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--dtype', choices=DTYPES, help='run one dtype in this process (child mode)')
  ap.add_argument('--small', action='store_true', help='toy sizes (a rehearsal of the script, not a measurement)')
  ap.add_argument('--timeout', type=int, default=240, help='seconds per dtype')
  ap.add_argument('--out', help='also write the JSON line to this file')
  args = ap.parse_args()
  if args.dtype:
    print('STENCIL_BENCH ' + json.dumps(run_dtype(args.dtype, args.small)), flush=True)
    return 0
  results, failed = [], None
  for name in DTYPES:
    cmd = ['timeout', '-k', '10', str(args.timeout), sys.executable, os.path.abspath(__file__), '--dtype', name]
    if args.small:
      cmd.append('--small')
    r = subprocess.run(cmd, capture_output=True, text=True)
    line = [l for l in r.stdout.splitlines() if l.startswith('STENCIL_BENCH ')]
    if r.returncode != 0 or not line:
      failed = {'dtype': name, 'exit': r.returncode, 'stderr': r.stderr[-2000:]}
      break  # nothing more is started on the GPU after a failure
    results.append(json.loads(line[-1][len('STENCIL_BENCH '):]))
    print('# %s done' % name, file=sys.stderr, flush=True)
  doc = {'tool': 'stencil_bench', 'warmup': WARMUP, 'steps': STEPS, 'small': bool(args.small),
         'workload': 'images (64, 3, 256, 256), 64 filters 4 x 4, 3 x (stencil, maxpool(2, 2))', 'dtypes': results}
  if failed:
    doc['failed'] = failed
  text = json.dumps(doc)
  print(text, flush=True)
  print(table(doc), file=sys.stderr, flush=True)
  if args.out:
    with open(args.out, 'w') as f:
      f.write(text + '\n')
  return 1 if failed else 0


if __name__ == '__main__':
  sys.exit(main())
