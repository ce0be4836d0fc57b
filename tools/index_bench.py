"""Measure ``spartan_amd.take`` / ``compress`` / ``a[mask]`` (spx_take,
spx_compact_count + spx_compact) against torch on one GPU.

Rows (fp32):
  take_rows      2^20 random rows of a (2^24, 128) array       torch.index_select(t, 0, i)
  take_axis1     a (32768, 32768) array along axis 1 by a
                 random permutation                             torch.index_select(t, 1, i)
  take_elem      2^26 random elements of a 1-d array of 2^28    torch.index_select(t, 0, i)
  mask_half      a[mask] on 2^28 elements, density 1/2          torch.masked_select
  mask_64th      a[mask] on 2^28 elements, density 1/64         torch.masked_select
  compress_rows  rows of (2^24, 128) at density 1/2             t[mask]

Each is timed with HIP events over 20 steps after 5 warm-up steps of the
forced expression -- the expression layer's host work, the count's read-back
and the allocation of the result are inside the timing -- and in the same
process the torch call runs on the same device tensors as the vendor figure.
The results are compared bit for bit in the same run.  ``tb_per_s`` is the
algorithmic bytes over the mean time: for take the index, the gathered rows
read and written; for compaction the input read once, the output written and
the mask counted TWICE (it is read by the count and by the compaction).

Every row runs in a child process of its own under ``timeout -k 10``; after
a failed child nothing more is started.  Prints one JSON line (and writes it
to --out).

  python tools/index_bench.py --out profiles/index_bench_<tag>.json
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = ['take_rows', 'take_axis1', 'take_elem', 'mask_half', 'mask_64th', 'compress_rows']
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
  return {'ms': round(sum(ms) / len(ms), 4), 'ms_median': round(ms[len(ms) // 2], 4), 'ms_min': round(ms[0], 4),
          'ms_max': round(ms[-1], 4)}


def _result_tensor(val):
  """The forced result as one device tensor (one worker: one tile, or a few
  uneven ones along one axis for a compaction)."""
  import torch
  tiles = sorted(val.local.items(), key=lambda kv: kv[0].ul)
  if len(tiles) == 1:
    return tiles[0][1].data
  axis = [d for d in range(len(val.shape)) if len({e.ul[d] for e, _ in tiles}) > 1][0]
  return torch.cat([t.data for _, t in tiles], dim=axis)


def run_config(name, small):
  import numpy as np
  import torch
  import spartan_amd
  from spartan_amd import backend, expr
  from spartan_amd.array import distarray
  spartan_amd.initialize()
  be = backend.get()
  assert isinstance(be, backend.HipBackend)
  sh = 8 if small else 0  # toy sizes: every power of two 8 smaller
  if name in ('take_rows', 'compress_rows'):
    shape = ((1 << 24) >> sh, 128)
  elif name == 'take_axis1':
    shape = (32768 >> (sh // 2), 32768 >> (sh // 2))
  else:
    shape = ((1 << 28) >> sh,)
  x = expr.rand(*shape, dtype=np.float32, seed=17).force()
  (ex, tile), = x.local.items()  # one worker: the whole array is one tile
  t = tile.data
  X = expr.lazify(x)
  g = torch.Generator(device=t.device)
  g.manual_seed(5)
  res = {'config': name, 'shape': list(shape)}

  def one_tile(dev):  # a device tensor as a one-tile array
    e = distarray.ext.from_shape(tuple(dev.shape))
    return expr.lazify(distarray.from_tiles(tuple(dev.shape), backend.np_dtype(dev.dtype), {e: 0}, {e: dev}))
  if name.startswith('take'):
    axis = 1 if name == 'take_axis1' else 0
    n = shape[axis]
    if name == 'take_axis1':
      idx = torch.randperm(n, device=t.device, generator=g)
    else:
      m = ((1 << 20) if name == 'take_rows' else (1 << 26)) >> sh
      idx = torch.randint(0, n, (m,), device=t.device, generator=g, dtype=torch.int64)
    I = one_tile(idx)
    m = idx.numel()
    row = int(np.prod(shape)) // n
    nbytes = 8 * m + 2 * 4 * m * row
    ours = lambda: expr.take(X, I, axis).force()
    vendor = lambda: torch.index_select(t, axis, idx)
    res.update(axis=axis, m=m, vendor='torch.index_select')
  else:
    n = shape[0]
    dens = 1.0 / 64 if name == 'mask_64th' else 0.5
    mask = torch.rand((n,), device=t.device, generator=g) < dens
    M = one_tile(mask)
    count = int(mask.sum().item())
    row = int(np.prod(shape)) // n
    nbytes = 4 * row * (n + count) + 2 * n
    if name == 'compress_rows':
      ours = lambda: expr.compress(M, X, 0).force()
      vendor = lambda: t[mask]
      res.update(vendor='t[mask]')
    else:
      ours = lambda: X[M].force()
      vendor = lambda: torch.masked_select(t, mask)
      res.update(vendor='torch.masked_select')
    res.update(density=dens, count=count, compact_tile=backend.COMPACT_TILE)
  # the two agree bit for bit
  got, want = _result_tensor(ours()), vendor()
  res['equal_torch'] = bool(got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32)))
  del got, want
  res['ours'] = _time(ours)
  res['torch'] = _time(vendor)
  res['algorithmic_bytes'] = nbytes
  for k in ('ours', 'torch'):
    res[k]['tb_per_s'] = round(nbytes / (res[k]['ms'] / 1e3) / 1e12, 3)
  res['ours_over_torch'] = round(res['ours']['ms'] / res['torch']['ms'], 3)
  return res


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--config', choices=CONFIGS, help='run one row in this process (child mode)')
  ap.add_argument('--small', action='store_true', help='toy sizes (a rehearsal of the script, not a measurement)')
  ap.add_argument('--timeout', type=int, default=150, help='seconds per row')
  ap.add_argument('--out', help='also write the JSON line to this file')
  args = ap.parse_args()
  if args.config:
    print('INDEX_BENCH ' + json.dumps(run_config(args.config, args.small)), flush=True)
    return 0
  results, failed = [], None
  for name in CONFIGS:
    cmd = ['timeout', '-k', '10', str(args.timeout), sys.executable, os.path.abspath(__file__), '--config', name]
    if args.small:
      cmd.append('--small')
    r = subprocess.run(cmd, capture_output=True, text=True)
    line = [l for l in r.stdout.splitlines() if l.startswith('INDEX_BENCH ')]
    if r.returncode != 0 or not line:
      failed = {'config': name, 'exit': r.returncode, 'stderr': r.stderr[-2000:]}
      break  # nothing more is started on the GPU after a failure
    results.append(json.loads(line[-1][len('INDEX_BENCH '):]))
    print('# %s done' % name, file=sys.stderr, flush=True)
  doc = {'tool': 'index_bench', 'dtype': 'float32', 'warmup': WARMUP, 'steps': STEPS, 'small': bool(args.small),
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
