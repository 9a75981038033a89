"""The Python front of the derivative entries (qp_batch_vjp / qp_batch_jvp, coneqp_batch_vjp / coneqp_batch_jvp, gp_batch_vjp /
gp_batch_jvp), written once: the check of a counting option, of `sol`, of the cotangent, of `wrt` and of the perturbations, the two
calls into the C entries and the shaping of the gradients.  An entry's module keeps its docstring, its option set, the problem
arguments under its name and the leading arguments of its C entries.  `rows` is the number of rows of G, h, s and z throughout.
The names of the data and the keys of `sol` are those of a QP unless an entry gives its own (gpbatchdiff: F and g lead, and the
solution has 'znl', 'snl', 'zl', 'sl'); vjp() and jvp() below are the calls of the entries whose C arguments are a QP's."""
import numpy as np

from . import _batch, _lib

EXIT_DONE, EXIT_SKIPPED, EXIT_FAILED = range(3)
MAX_REFINEMENT = 3
WRT = ("P", "q", "G", "h", "A", "b")


def count(who, name, v, hi):
    """options[name] as a nonnegative integer of at most hi."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 0:
        raise ValueError("options['%s'] must be a nonnegative integer" % name)
    if v > hi:
        raise ValueError("%s: options['%s'] = %d is outside its limit 0 <= %s <= %d" % (who, name, v, name, hi))
    return int(v)


def problem(who, entry, prepare, *args):
    """The forward entry's own checks of the problem arguments, under the derivative entry's name."""
    try:
        _, sizes, data = prepare(*args, None)
    except ValueError as e:
        raise ValueError(str(e).replace(entry + ":", who + ":", 1)) from None
    return sizes, data


def solution(sol, entry, B, n, rows, p, copy=False, keys=None):
    """x, y, s, z and exit of `sol` as contiguous arrays, one member after the other; copy: arrays of their own in every case.
    keys: the (key, rows) pairs of an entry whose solution has other vectors."""
    keys = (("x", n), ("y", p), ("s", rows), ("z", rows)) if keys is None else tuple(keys)
    if not isinstance(sol, dict) or any(k not in sol for k in [k for k, _ in keys] + ["exit"]):
        raise TypeError("'sol' must be the dictionary %s returned, with %s and 'exit'" % (entry, ", ".join(repr(k) for k, _ in keys)))
    out = []
    for k, r in keys:
        v = np.asarray(sol[k], dtype=np.float64)
        if v.shape != (r, B):
            raise TypeError("sol['%s'] must be a 'd' matrix of size (%d, %d)" % (k, r, B))
        out.append((np.array(v.T, order="C") if copy else np.ascontiguousarray(v.T)).reshape(-1))
    code = np.asarray(sol["exit"])
    if code.shape != (B,) or code.dtype.kind not in "iu":
        raise TypeError("sol['exit'] must be an integer array of length %d" % B)
    return out, (np.array(code, dtype=np.int64) if copy else np.ascontiguousarray(code, dtype=np.int64))


def strides(data):
    """The member strides of P, G, h, A, b in the data of a _prepare with P, q, G, h, A, b."""
    return [data[k][1] for k in (0, 2, 3, 4, 5)]


def solution_pointers(vecs, code, p):
    x, y, s, z = vecs
    return [_lib.pd(x), _lib.pd(y) if p else None, _lib.pd(s), _lib.pd(z), _lib.pi(code)]


def _perturbation(name, v, is_matrix, n, B, rows, defines):
    """(values or None, member stride) of one perturbation, checked as the forward entry checks the datum it perturbs."""
    if v is None:
        return None, 0
    if is_matrix:
        vals, stride, _ = _batch.matrix(v, name, n, B, rows=rows, defines=defines)
        return vals, stride
    return _batch.shared_or_batch(v, name, rows, B, "'%s' must be a 'd' matrix of size (%d,1)" % (name, rows))


def from_members(v, shared, rows, n, B):
    """A matrix gradient as the C entry wrote it -- column-major, one member after the other -- in the argument's shape."""
    return np.ascontiguousarray(v.reshape(n, rows).T) if shared else np.ascontiguousarray(v.reshape(B, n, rows).transpose(0, 2, 1))


def column_gradient(g, given, shared, done):
    """The gradient of h or b: per member, or the sum over the done members in the shape the shared column was given."""
    if not shared:
        return g
    t = g[:, done].sum(axis=1)
    return t.reshape(-1, 1) if isinstance(given, np.ndarray) and given.ndim == 2 else t


def _extra_pointers(extra):
    return [_lib.pi(v) if v.dtype == np.int64 else _lib.pd(v) for v in extra.values()]


def cotangent(gx, n, B):
    """gx checked, one member after the other."""
    g = _batch.columns(gx, "gx", "one column per member")
    if g.shape != (n, B):
        raise TypeError("'gx' must be a 'd' matrix of size (%d, %d)" % (n, B))
    return np.ascontiguousarray(g.T).reshape(-1)


def named(who, wrt, names=WRT):
    """wrt as a tuple of the entry's data names."""
    wrt = (wrt,) if isinstance(wrt, str) else tuple(wrt)
    if any(k not in names for k in wrt):
        raise ValueError("%s: wrt names %s; it takes %s" % (who, ", ".join(repr(k) for k in wrt if k not in names),
                                                            ", ".join(repr(k) for k in names)))
    return wrt


def vjp(symbol, who, common, strides, B, n, rows, p, gx, wrt, h, b, extra=None):
    """gx and wrt checked, the C entry `symbol` on common() + cotangent + results + extra + exit, and the result dictionary.
    strides: those of P, G, h, A, b.  extra: further per-member results by their keys, in the order of the C entry."""
    gv = cotangent(gx, n, B)
    wrt = named(who, wrt)
    sP, sG, sh, sA, sb = strides
    L = _lib.lib()
    ux, uy, uz = (np.zeros((r, B), order="F") for r in (n, p, rows))
    gexit = np.zeros(B, dtype=np.int64)
    extra = dict(extra or {})
    shapes = {"P": (n, sP), "G": (rows, sG), "A": (p, sA)}
    mats = {k: np.zeros((B if stride else 1) * r * n) if k in wrt and r else None for k, (r, stride) in shapes.items()}
    args = common() + [_lib.pd(gv), _lib.pd(ux), _lib.pd(uy) if p else None, _lib.pd(uz)]
    args += [None if mats[k] is None else _lib.pd(mats[k]) for k in ("P", "G", "A")] + _extra_pointers(extra) + [_lib.pi(gexit)]
    _lib.raise_for(getattr(L, symbol)(*args), symbol)
    out = {"ux": ux, "uy": uy, "uz": uz, "exit": gexit, **extra}
    done = gexit == EXIT_DONE
    for k in wrt:
        if k == "q":
            out[k] = ux.copy()
        elif k == "h":
            out[k] = column_gradient(0.0 - uz, h, sh == 0, done)                    # 0 - u: no negative zeros
        elif k == "b":
            out[k] = column_gradient(0.0 - uy, b, sb == 0, done) if p else None
        else:
            r, stride = shapes[k]
            out[k] = None if mats[k] is None else from_members(mats[k], stride == 0, r, n, B)
    return out


def perturbations(given, B, n, rows, p, names=WRT, sizes=None, defines="q"):
    """The six perturbations, checked, as (values or None, member stride) pairs.  names, sizes, defines: the data of an entry that
    is not a QP, their rows, and the argument whose columns are the members; a name in upper case is a matrix."""
    sizes = (n, n, rows, rows, p, p) if sizes is None else sizes
    return [_perturbation("d" + k, v, k.isupper(), n, B, r, defines) for k, v, r in zip(names, given, sizes)]


def jvp(symbol, common, pert, B, n, rows, p, extra=None):
    """The C entry `symbol` on common() + perturbations + results + extra + exit, and the result dictionary."""
    L = _lib.lib()
    dx, dy, dz, ds = (np.zeros((r, B), order="F") for r in (n, p, rows, rows))
    gexit = np.zeros(B, dtype=np.int64)
    extra = dict(extra or {})
    args = common()
    for k, (vals, stride) in zip(WRT, pert):
        args += [None if vals is None or (k in "Ab" and not p) else _lib.pd(vals), stride]
    args += [_lib.pd(dx), _lib.pd(dy) if p else None, _lib.pd(dz), _lib.pd(ds)] + _extra_pointers(extra) + [_lib.pi(gexit)]
    _lib.raise_for(getattr(L, symbol)(*args), symbol)
    return {"x": dx, "y": dy, "z": dz, "s": ds, "exit": gexit, **extra}
