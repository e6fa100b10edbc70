"""An eager NumPy stand-in for the TensorFlow 1.x calls that the reference's warp and loss code makes.

TEST INFRASTRUCTURE ONLY, and only ever installed in a CHILD process (oracle/run_reference.py): `install()` puts the object built
here into sys.modules as `tensorflow` (+ the `tensorflow.contrib...` submodules the reference imports, an inert `cv2`, and
`scipy.misc` where it is absent) so that the reference's files can be imported unchanged from their checkout and their graph-building
functions compute values at once on NumPy arrays.  It is NOT a package named tensorflow on any import path, and a test process never
calls install().

Written from the TF 1.x op documentation and this project's notes; one line of semantics beside each op.  A "tensor" is a NumPy
array (or scalar); Python operators on tensors are NumPy's, which for float32 arrays round once per operation as every elementwise
TF CPU kernel does (Python numbers are "weak": they take the array's type first, as TF's constant conversion does).

Two modes (`set_mode`):
  f32   every op rounds once to float32 -- what the TF CPU kernels of the reference's graph compute.
  f64   the same text in float64: 'float32' casts, float constants, linspace, eye, ones/zeros and fed values are float64, integers
        stay int32 -- the high-precision value of the reference's own formulas.

Where a choice exists:
  cast float -> int32   truncates; out of range / NaN -> INT_MIN (x86 cvttss2si / cvttsd2si), as oracle cast_i32_x86.
  round                 half to even.
  linspace              start + i * ((stop - start) / (n - 1)) in the working type.
  matmul                in-order multiply-then-add over k, no FMA (integer matmul: exact).
  add_n                 left to right (Eigen's in0 + in1 + ... expression of the AddN kernel for up to 8 inputs).
  matrix_inverse        THE ONE OP TAKEN ON TRUST.  TF calls Eigen's PartialPivLU, which is not here to be run: in f32 mode this is
                        oracle.stabnet_oracle.inv8_partial_piv_lu -- an ASSUMPTION CARRIED OVER from the oracle, so a run of the
                        reference through this module cannot disprove it (tests/test_oracle_independent_cpu.py checks its pivot
                        sequence against SciPy's).  In f64 mode it is numpy.linalg.inv.
  reduce_mean / reduce_sum   TF's summation order is unspecified.  Here: accumulate in float64, round once.  Nothing downstream may
                        depend on that: comparisons of reduced values carry a summation bar built from `reduce_log`.
  placeholder           returns the value fed under its name (`feeds`); an unnamed one gets TF's default name: Placeholder,
                        Placeholder_1, ... in creation order.
  get_collection        returns what the caller registered in `collections`.
  variable_scope, name_scope, control_dependencies, group, summary.*, Print, add_to_collection: inert.

Three logs let the caller state facts about a run without reading any reference internals:
  trace       every DECISION in call order: where conditions, minimum / maximum / clip_by_value sides, float -> int casts (floor,
              round), ties met by round, gather indices, the sign under abs.  Two runs with equal traces evaluated the same smooth piece.
  where_log   the condition array of every tf.where.
  reduce_log  per reduce_mean / reduce_sum: (input array, axes).
"""
import contextlib
import sys
import types

import numpy as np

INT_MIN = np.int32(-2147483648)


class _State:
    def __init__(self):
        self.W = np.float32          # the working float type
        self.feeds = {}
        self.collections = {}
        self.n_placeholders = 0
        self.trace = []
        self.where_log = []
        self.reduce_log = []
        self.inv_f32 = None


def _build():
    S = _State()
    tf = types.ModuleType("tensorflow")
    tf.__doc__ = "eager NumPy stand-in (tests/tf_eager_standin.py)"
    tf._state = S
    tf.float32 = "float32"
    tf.int32 = "int32"

    def set_mode(mode):
        S.W = {"f32": np.float32, "f64": np.float64}[mode]

    def reset(feeds=None, collections=None):
        S.feeds = dict(feeds or {})
        S.collections = dict(collections or {})
        S.n_placeholders = 0
        S.trace, S.where_log, S.reduce_log = [], [], []

    tf.set_mode, tf.reset = set_mode, reset

    def _decide(kind, a):
        S.trace.append((kind, np.ascontiguousarray(a)))

    def _shape(shape):
        return tuple(int(v) for v in np.asarray(shape).reshape(-1))

    def _fdtype(dtype):
        """A dtype argument -> NumPy type; float32 means the working type."""
        name = dtype if isinstance(dtype, str) else np.dtype(dtype).name
        if name == "float32":
            return S.W
        if name == "int32":
            return np.int32
        raise NotImplementedError("dtype %r" % (dtype,))

    def _t(x):
        """Python numbers / lists -> tensors of the working float type or int32; arrays as they are."""
        if isinstance(x, (np.ndarray, np.generic)):
            return x
        a = np.asarray(x)
        if a.dtype.kind == "f":
            return a.astype(S.W)
        if a.dtype.kind in "iu":
            return a.astype(np.int32)
        return a

    # ---- shapes and data movement (exact) ------------------------------------------------------------------------------
    tf.shape = lambda x: list(np.shape(x))                                   # shape as Python ints (eager: static = dynamic)
    tf.reshape = lambda x, shape, name=None: np.reshape(_t(x), _shape(shape))  # row-major reshape, one -1 allowed

    def slice_(x, begin, size):                                              # x[begin : begin + size] per axis, size -1 = to the end
        x = _t(x)
        idx = tuple(slice(int(b), None if int(s) == -1 else int(b) + int(s)) for b, s in zip(begin, size))
        return x[idx]
    tf.slice = slice_
    tf.concat = lambda values, axis, name=None: np.concatenate([_t(v) for v in values], axis=axis)
    tf.stack = lambda values, axis=0: np.stack([_t(v) for v in values], axis=axis)
    tf.tile = lambda x, multiples: np.tile(_t(x), _shape(multiples))
    tf.transpose = lambda x, perm=None: np.transpose(_t(x), perm)
    tf.expand_dims = lambda x, axis: np.expand_dims(_t(x), axis)
    tf.ones = lambda shape, dtype="float32": np.ones(_shape(shape), _fdtype(dtype))
    tf.zeros = lambda shape, dtype="float32": np.zeros(_shape(shape), _fdtype(dtype))
    tf.ones_like = lambda x: np.ones_like(_t(x))
    tf.eye = lambda n: np.eye(int(n), dtype=S.W)
    tf.range = lambda n: np.arange(int(n), dtype=np.int32)
    tf.stop_gradient = lambda x: x

    def constant(value, dtype=None, shape=None):                             # a scalar fills `shape`; a list is reshaped to it
        a = np.asarray(value)
        if dtype is not None:
            a = a.astype(_fdtype(dtype))
        else:
            a = _t(a)
        if shape is not None:
            shape = _shape(shape)
            a = np.full(shape, a, a.dtype) if a.ndim == 0 else a.reshape(shape)
        return a
    tf.constant = constant

    def gather(params, indices):                                             # params[indices] along axis 0; TF's CPU kernel refuses
        params, indices = _t(params), np.asarray(indices)                    # an index out of range, so does this
        if indices.size and (indices.min() < 0 or indices.max() >= params.shape[0]):
            raise IndexError("gather: index out of range [0, %d)" % params.shape[0])
        _decide("gather", indices.astype(np.int64))
        return params[indices]
    tf.gather = gather

    # ---- elementwise ------------------------------------------------------------------------------------------------------
    def cast(x, dtype):
        x = _t(x)
        T = _fdtype(dtype)
        if T is np.int32 and np.asarray(x).dtype.kind == "f":                # truncate; out of range / NaN -> INT_MIN (cvtts[sd]2si)
            xa = np.asarray(x)
            ok = (xa >= -2147483648.0) & (xa < 2147483648.0)
            out = np.where(ok, np.where(ok, xa, 0).astype(np.int32), INT_MIN).astype(np.int32)
            _decide("cast_i32", out)
            return out if xa.ndim else np.int32(out)
        return np.asarray(x).astype(T) if np.ndim(x) else T(x)
    tf.cast = cast
    tf.floor = lambda x: np.floor(_t(x))
    def round_(x):                                                           # half to even
        x = _t(x)
        _decide("round_tie", x - np.floor(x) == 0.5)
        return np.rint(x)
    tf.round = round_

    def abs_(x):
        x = _t(x)
        _decide("abs", np.sign(x).astype(np.int8))
        return np.abs(x)
    tf.abs = abs_
    tf.div = lambda a, b: _t(a) / _t(b)                                      # float operands here: true division
    tf.greater = lambda a, b: np.greater(_t(a), _t(b))
    tf.logical_or = lambda a, b: np.logical_or(a, b)

    def where(cond, a, b):                                                   # elementwise select
        cond = np.asarray(cond, bool)
        _decide("where", cond)
        S.where_log.append(cond.copy())
        return np.where(cond, _t(a), _t(b))
    tf.where = where

    def _as_w(v, like):
        """A Python number beside a tensor takes the tensor's type (TF's constant conversion)."""
        return np.asarray(like).dtype.type(v) if not isinstance(v, (np.ndarray, np.generic)) else v

    def minimum(a, b):
        a = _t(a)
        b = _as_w(b, a)
        _decide("minimum", np.less(a, b))
        return np.minimum(a, b)

    def maximum(a, b):
        a = _t(a)
        b = _as_w(b, a)
        _decide("maximum", np.greater(a, b))
        return np.maximum(a, b)

    def clip_by_value(x, lo, hi):                                            # min(max(x, lo), hi)
        x = _t(x)
        lo, hi = _as_w(lo, x), _as_w(hi, x)
        _decide("clip", np.less(x, lo).astype(np.int8) - np.greater(x, hi).astype(np.int8))
        return np.minimum(np.maximum(x, lo), hi)
    tf.minimum, tf.maximum, tf.clip_by_value = minimum, maximum, clip_by_value

    def linspace(start, stop, num):                                          # start + i * ((stop - start) / (n - 1)), working type
        W = S.W
        start, stop, num = W(start), W(stop), int(num)
        if num == 1:
            return np.array([start], W)
        step = (stop - start) / W(num - 1)
        return start + step * np.arange(num, dtype=W)
    tf.linspace = linspace

    def add_n(values):                                                       # left to right
        out = _t(values[0])
        for v in values[1:]:
            out = out + _t(v)
        return out
    tf.add_n = add_n

    # ---- linear algebra ---------------------------------------------------------------------------------------------------
    def matmul(a, b):
        a, b = _t(a), _t(b)
        if a.dtype.kind in "iu":                                             # integer: exact
            return np.matmul(a, b)
        out = a[..., :, 0, None] * b[..., None, 0, :]                        # in-order multiply-then-add over k, one rounding each
        for k in range(1, a.shape[-1]):
            out = out + a[..., :, k, None] * b[..., None, k, :]
        return out
    tf.matmul = matmul

    def matrix_inverse(A):
        A = _t(A)
        if S.W is np.float64:
            return np.linalg.inv(A)
        if S.inv_f32 is None:                                                # ASSUMPTION CARRIED OVER (module docstring)
            from oracle.stabnet_oracle import inv8_partial_piv_lu
            S.inv_f32 = inv8_partial_piv_lu
        return S.inv_f32(A.reshape((-1,) + A.shape[-2:])).reshape(A.shape)
    tf.matrix_inverse = matrix_inverse

    # ---- reductions (order unspecified in TF: float64 accumulation, one rounding) -------------------------------------------
    def _reduce(x, axis, mean):
        x = _t(x)
        ax = None if axis is None else tuple(int(a) for a in np.atleast_1d(axis))
        S.reduce_log.append((x.copy(), ax))
        f = np.mean if mean else np.sum
        r = f(x.astype(np.float64), axis=ax)
        return x.dtype.type(r) if np.ndim(r) == 0 else r.astype(x.dtype)
    tf.reduce_mean = lambda x, axis=None: _reduce(x, axis, True)
    tf.reduce_sum = lambda x, axis=None: _reduce(x, axis, False)

    # ---- graph plumbing ---------------------------------------------------------------------------------------------------
    def placeholder(dtype, shape=None, name=None):
        if name is None:
            name = "Placeholder" if S.n_placeholders == 0 else "Placeholder_%d" % S.n_placeholders
            S.n_placeholders += 1
        if name not in S.feeds:
            raise KeyError("placeholder %r was not fed" % name)
        v = np.asarray(S.feeds[name])
        T = _fdtype(dtype)
        return v.astype(T) if v.ndim else T(v)
    tf.placeholder = placeholder
    tf.get_collection = lambda key: list(S.collections.get(key, []))
    tf.add_to_collection = lambda key, value: None
    tf.GraphKeys = types.SimpleNamespace(REGULARIZATION_LOSSES="regularization_losses", UPDATE_OPS="update_ops")

    @contextlib.contextmanager
    def _scope(*a, **k):
        yield
    tf.variable_scope = tf.name_scope = tf.control_dependencies = _scope
    tf.group = lambda *a, **k: None
    tf.Print = lambda x, *a, **k: x
    tf.summary = types.SimpleNamespace(image=lambda *a, **k: None, scalar=lambda *a, **k: None, histogram=lambda *a, **k: None)

    # ---- what the import chain touches at import time, none of whose arithmetic is wanted ------------------------------------
    class _Flags:
        """tf.app.flags: DEFINE_* store their default, FLAGS.<name> reads it."""

        def __init__(self):
            self.FLAGS = types.SimpleNamespace()
            for kind in ("string", "integer", "float", "boolean"):
                setattr(self, "DEFINE_" + kind, self._define)

        def _define(self, name, default, help=None):
            setattr(self.FLAGS, name, default)
    tf.app = types.SimpleNamespace(flags=_Flags())

    def _refuse(name):
        def f(*a, **k):
            raise NotImplementedError("tf stand-in: %s is cut at the library boundary; the caller supplies its result" % name)
        return f

    contrib = types.ModuleType("tensorflow.contrib")
    layers = types.ModuleType("tensorflow.contrib.layers")
    layers.xavier_initializer = lambda *a, **k: None
    layers.l2_regularizer = lambda *a, **k: None
    slim = types.ModuleType("tensorflow.contrib.slim")
    slim.arg_scope = _scope
    slim.fully_connected = _refuse("slim.fully_connected")
    nets = types.ModuleType("tensorflow.contrib.slim.nets")
    resnet_v2 = types.ModuleType("tensorflow.contrib.slim.nets.resnet_v2")
    resnet_v2.resnet_arg_scope = lambda *a, **k: None
    resnet_v2.resnet_v2_50 = _refuse("resnet_v2.resnet_v2_50")
    nets.resnet_v2 = resnet_v2
    slim.nets = nets
    contrib.layers, contrib.slim = layers, slim
    tf.contrib = contrib
    for name in ("uniform_unit_scaling_initializer", "zeros_initializer", "constant_initializer", "truncated_normal_initializer",
                 "random_normal_initializer"):
        setattr(tf, name, lambda *a, **k: None)

    def __getattr__(name):
        raise AttributeError("tf stand-in: tf.%s is not among the ops of the reference's warp and loss code" % name)
    tf.__getattr__ = __getattr__
    modules = {"tensorflow": tf, "tensorflow.contrib": contrib, "tensorflow.contrib.layers": layers, "tensorflow.contrib.slim": slim,
               "tensorflow.contrib.slim.nets": nets, "tensorflow.contrib.slim.nets.resnet_v2": resnet_v2}
    return tf, modules


def install():
    """CHILD PROCESSES ONLY.  Put the stand-in into sys.modules as tensorflow(.contrib...), with an inert cv2 and, where scipy has none,
    an inert scipy.misc.  -> the tensorflow stand-in (set_mode / reset / _state on it)."""
    if "tensorflow" in sys.modules:
        raise RuntimeError("a tensorflow module is already imported in this process")
    tf, modules = _build()
    sys.modules.update(modules)
    if "cv2" not in sys.modules:
        sys.modules["cv2"] = types.ModuleType("cv2")                          # imported by the chain, never called by what is run
    try:
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            import scipy.misc  # noqa: F401
    except ImportError:
        pkg = sys.modules.setdefault("scipy", types.ModuleType("scipy"))
        pkg.misc = sys.modules["scipy.misc"] = types.ModuleType("scipy.misc")
    return tf
