"""Measure spx_nbody_accel on one GPU.

Legs: float32 and float64, n in {2^13, 2^15, 2^16, 2^17} bodies on the unit
scale of the tests (positions uniform in [-50, 50]^3, masses in [1, 2], G = 1,
rmin = 1), built on the device from a seed:

  spx     HipBackend.nbody_accel: the all-pairs kernel and, where the plan
          splits the sources, the sum of the partials;

  torch   the composition a user of the parent commit, which has no n-body
          kernel, had, on the same GPU in the same run: (chunk, n) blocks of
          dx, dy, dz, r2 = dx^2 + dy^2 + dz^2, clamp(r2, rmin^2), rsqrt, its
          cube times m, and three weighted row sums, with the chunk chosen so
          that one block holds 2^25 elements.  The un-chunked composition of
          the expression layer does not fit at these sizes.

Both are timed with HIP events after warm-up, in interleaved rounds in one
process (round r runs every leg once), and report the median and the minimum.
Before anything is timed the two routes are compared on the same input:
``diff`` is the largest |a_spx - a_torch| / S_torch over all elements, S the
sum of the terms' magnitudes.

``Gint/s`` is n^2 interactions over the spx median.  ``of_peak`` multiplies it
by the kernel's own inner-loop operation count per interaction -- 18 in
float32 (3 subtractions, 1 multiply and 2 multiply-adds for r^2, 1 reciprocal
square root counted as ONE operation, 3 multiplies, 3 multiply-adds; the
compare and select of the clamp are not counted), 29 in float64 (the same
plus the two Newton steps on v_rsq_f64: 1 + 2 * (1 multiply + 2 multiply-adds)
= 11) -- and divides by the vector peak of the dtype (157.3 TFLOP/s float32,
78.6 TFLOP/s float64).

``--lib PATH`` times another build of the library (for instance one compiled
with -DSPX_NBODY_SCALAR_SRC=1, the scalar-load variant of the source reads).

One child process per dtype, under ``timeout -k 10``, which signals the
child's whole process group; after a child that fails or runs past its limit
nothing more is started on the GPU: the table so far is written and the tool
exits 1.  Nothing here asserts a speed.

  python tools/nbody_bench.py --out profiles/nbody_bench.txt
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (1 << 13, 1 << 15, 1 << 16, 1 << 17)
DTYPES = ('float32', 'float64')
PEAK = {'float32': 157.3e12, 'float64': 78.6e12}
FLOPS = {'float32': 18, 'float64': 29}
BLOCK = 1 << 25  # elements of one (chunk, n) block of the torch composition
G, RMIN = 1.0, 1.0


def data(n, dtype, seed=0):
  import torch
  g = torch.Generator(device='cuda')
  g.manual_seed(seed + n)
  dt = getattr(torch, dtype)
  x, y, z = (torch.rand((n,), generator=g, device='cuda', dtype=dt) * 100 - 50 for _ in range(3))
  return x, y, z, torch.rand((n,), generator=g, device='cuda', dtype=dt) + 1


def torch_accel(x, y, z, m, want_S=False):
  """(ax, ay, az) -- and S with ``want_S`` -- by the torch composition, a chunk of targets at a time."""
  import torch
  n = x.shape[0]
  chunk = max(1, BLOCK // n)
  out = [torch.empty_like(x) for _ in range(3)]
  S = [torch.empty_like(x) for _ in range(3)] if want_S else None
  gm = (G * m)[None, :]
  for lo in range(0, n, chunk):
    hi = min(lo + chunk, n)
    d = [p[None, :] - p[lo:hi, None] for p in (x, y, z)]
    r2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2]
    inv = torch.rsqrt(torch.clamp(r2, min=RMIN * RMIN))
    w = gm * inv * inv * inv
    for c in range(3):
      f = w * d[c]
      out[c][lo:hi] = f.sum(dim=1)
      if want_S:
        S[c][lo:hi] = f.abs().sum(dim=1)
  return (out, S) if want_S else out


def child(dtype, sizes, rounds, warmup, lib):
  """One dtype: every size, both routes; one JSON line a size on stdout."""
  import torch
  import spartan_amd
  from spartan_amd import backend, binding
  if lib:
    binding.load_library(lib)
  spartan_amd.initialize()
  be = backend.get()
  legs, rows = [], {}
  for n in sizes:
    x, y, z, m = data(n, dtype)
    got = be.nbody_accel(x, y, z, x, y, z, m, G, RMIN)
    ref, S = torch_accel(x, y, z, m, want_S=True)
    torch.cuda.synchronize()
    diff = max(float(((a - b).abs() / s).max().item()) for a, b, s in zip(got, ref, S))
    rows[n] = {'dtype': dtype, 'n': n, 'device': torch.cuda.get_device_name(0), 'diff': diff,
               'splits': binding.nbody_plan(dtype, n, n)[1]}
    legs.append((n, 'spx', (lambda x=x, y=y, z=z, m=m: be.nbody_accel(x, y, z, x, y, z, m, G, RMIN))))
    legs.append((n, 'torch', (lambda x=x, y=y, z=z, m=m: torch_accel(x, y, z, m))))
  times = {i: [] for i in range(len(legs))}
  for r in range(warmup + rounds):
    for i, leg in enumerate(legs):
      a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      a.record()
      leg[2]()
      b.record()
      b.synchronize()
      if r >= warmup:
        times[i].append(a.elapsed_time(b))
  for i, (n, which, _fn) in enumerate(legs):
    rows[n][which] = {'median': statistics.median(times[i]), 'min': min(times[i]), 'runs': len(times[i])}
  for n in sizes:
    print('NBODY_BENCH ' + json.dumps(rows[n]))


def run_child(dtype, args):
  """The child's rows, or a string saying why there are none."""
  cmd = ['timeout', '-k', '10', str(args.child_timeout), sys.executable, os.path.abspath(__file__), '--child', dtype,
         '--rounds', str(args.rounds), '--warmup', str(args.warmup), '--sizes'] + [str(n) for n in args.sizes]
  if args.lib:
    cmd += ['--lib', args.lib]
  with tempfile.TemporaryFile() as f:  # a file, not a pipe: nothing is held open by a killed child
    r = subprocess.run(cmd, stdin=subprocess.DEVNULL, stdout=f, stderr=subprocess.STDOUT)
    f.seek(0)
    text = f.read().decode(errors='replace')
  if r.returncode != 0:
    why = 'ran past %d s' % args.child_timeout if r.returncode in (124, 137) else 'exited %d' % r.returncode
    return 'child %s: %s' % (why, text[-300:])
  rows = [json.loads(line[len('NBODY_BENCH '):]) for line in text.splitlines() if line.startswith('NBODY_BENCH ')]
  return rows if len(rows) == len(args.sizes) else 'child printed %d of %d rows: %s' % (len(rows), len(args.sizes),
                                                                                     text[-300:])


def main():
  ap = argparse.ArgumentParser()
  ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'nbody_bench.txt'))
  ap.add_argument('--rounds', type=int, default=9)
  ap.add_argument('--warmup', type=int, default=2)
  ap.add_argument('--sizes', type=int, nargs='*', default=list(SIZES))
  ap.add_argument('--child-timeout', type=int, default=240)
  ap.add_argument('--lib', default=None, help='another build of libspx.so to time')
  ap.add_argument('--child', metavar='DTYPE', help='child mode: time one dtype and exit')
  args = ap.parse_args()
  if args.child:
    child(args.child, args.sizes, args.rounds, args.warmup, args.lib)
    return 0
  rows, failed, device = [], None, '?'
  for i, dtype in enumerate(DTYPES):
    sys.stderr.write('nbody_bench: %s\n' % dtype)
    got = run_child(dtype, args)
    if isinstance(got, str):
      failed = (dtype, got, DTYPES[i + 1:])
      break  # nothing more is started on the GPU after a failure
    rows += got
    device = got[0]['device']
  lines = ['nbody_bench: %s, %d rounds after %d warm-up, HIP events; times in ms%s'
           % (device, args.rounds, args.warmup, '; library %s' % os.path.basename(args.lib) if args.lib else ''),
           'torch: (chunk, n) blocks of dx dy dz, r2, clamp, rsqrt, w = G m inv^3, three row sums; chunk = 2^25 / n',
           'of_peak: n^2 x %d (float32) / %d (float64) operations over the spx median and the vector peak' %
           (FLOPS['float32'], FLOPS['float64']), '',
           '%-8s %8s %6s %10s %10s %11s %10s %9s %8s %9s' % ('dtype', 'n', 'splits', 'spx med', 'spx min', 'torch med',
                                                        'torch/spx', 'Gint/s', 'of_peak', 'diff')]
  for row in rows:
    spx, tor = row['spx'], row['torch']
    rate = float(row['n']) ** 2 / (spx['median'] * 1e-3)
    lines.append('%-8s %8d %6d %10.3f %10.3f %11.3f %10.2f %9.1f %7.1f%% %9.2e'
                 % (row['dtype'], row['n'], row['splits'], spx['median'], spx['min'], tor['median'],
                    tor['median'] / spx['median'], rate / 1e9, 100 * rate * FLOPS[row['dtype']] / PEAK[row['dtype']],
                    row['diff']))
  if failed is not None:
    lines.append('%s: not measured: %s' % failed[:2])
    if failed[2]:
      lines.append('not started after that failure: %s' % ', '.join(failed[2]))
  text = '\n'.join(lines)
  print(text)
  with open(args.out, 'w') as f:
    f.write(text + '\n')
  return 0 if failed is None else 1


if __name__ == '__main__':
  sys.exit(main())
