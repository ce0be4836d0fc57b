"""Dev-tool helper: build a patched variant of libspx.so by text substitution
on a copy of the sources (the product source carries no switches).

  from spx_variant import Variant
  v = Variant('name')   # copies spartan_amd/csrc/ and include/ to tools/bin/name_src/
  v.sub(old, new)       # old must occur exactly once across the copied files
  v.count(text)         # occurrences across the copied files
  v.build()             # the product's hipcc flags -> tools/bin/libspx_name.so

The copy keeps the tree's relative layout, so no #include needs rewriting and
a new header under csrc/ is picked up without touching the tools.  The build
needs no GPU.  As a command it applies one substitution:
  python3 tools/spx_variant.py NAME 'old text' 'new text'"""
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from __graft_entry__ import HIPCC_FLAGS  # noqa: E402  (the product flags)

COPIED = ('spartan_amd/csrc', 'include')


class Variant:
  def __init__(self, name):
    self.name = name
    self.bin = os.path.join(ROOT, 'tools', 'bin')
    self.src = os.path.join(self.bin, name + '_src')
    shutil.rmtree(self.src, ignore_errors=True)
    for d in COPIED:
      shutil.copytree(os.path.join(ROOT, d), os.path.join(self.src, d))
    self.files = sorted(os.path.join(self.src, d, f) for d in COPIED for f in os.listdir(os.path.join(self.src, d)))

  def _texts(self):
    return [(f, open(f).read()) for f in self.files]

  def count(self, text):
    return sum(s.count(text) for _, s in self._texts())

  def sub(self, old, new):
    """Replace ``old``, which must occur exactly once across the copied files."""
    hits = [(f, s) for f, s in self._texts() if old in s]
    n = sum(s.count(old) for _, s in hits)
    assert n == 1, '%s: anchor %r found %d times' % (self.name, old[:60], n)
    f, s = hits[0]
    open(f, 'w').write(s.replace(old, new))

  def build(self):
    csrc = os.path.join(self.src, 'spartan_amd', 'csrc')
    out = os.path.join(self.bin, 'libspx_%s.so' % self.name)
    hipcc = os.path.join(os.environ.get('ROCM_PATH', '/opt/rocm'), 'bin', 'hipcc')
    subprocess.run([hipcc] + HIPCC_FLAGS + ['-o', out + '.tmp'] +
                   [os.path.join(csrc, f) for f in ('spx.hip', 'tiling.cpp', 'comm.cpp')] + ['-ldl'], check=True)
    os.replace(out + '.tmp', out)
    shutil.rmtree(self.src)
    print('built tools/bin/libspx_%s.so' % self.name)
    return out


if __name__ == '__main__':
  v = Variant(sys.argv[1])
  v.sub(sys.argv[2], sys.argv[3])
  v.build()
