"""spartan_amd.expr -- the spartan.expr API (spartan/expr/__init__.py:26-53)
on the MI355X tile-execution backend."""
from .base import (Expr, NotShapeable, as_array, eager, evaluate, force, glom, lazify, newaxis,
                   optimized_dag)
from .builtins import (abs, add, arange, argmax, argmin, astype, bincount, concatenate, count_nonzero,
                       count_zero, exp,
                       ln, log, maximum, max, mean, min, minimum, multiply, norm, ones, power, rand, randn,
                       size, sqrt, square, std, sub, sum, zeros)
from .affinity import normalized_affinity, pairwise_kernel
from .dot import dot
from .eigh import eigh, eigvalsh
from .filter import compress, take
from .fuzzy import fuzzy_assign, fuzzy_membership
from .graph import shortest_path
from .join import map2, outer
from .linalg import cho_solve, cholesky, solve_triangular
from .map import map
from .map_with_location import map_with_location, region_map
from .nbody import nbody_accel
from .ndarray import ndarray
from .qr import qr
from .reduce import reduce
from .reshape import reshape
from .scan import scan
from .slice import slice_expr
from .sort import argpartition, argsort, partition, sort
from .sparse import sparse_diagonal, sparse_empty, sparse_rand, sparse_transpose, todense
from .svd import pinv, svd, svdvals
from .topk import argtopk, topk
from .transpose import transpose
from .write_array import from_file, from_numpy, write
from . import stencil  # the submodule, as in the reference: stencil.stencil / stencil.maxpool

Expr.outer = outer
Expr.sum = sum
Expr.mean = mean
Expr.astype = astype
Expr.argmin = argmin
Expr.argmax = argmax
