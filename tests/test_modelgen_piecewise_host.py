"""CPU tests of the piecewise operations of vihds.modelgen (conditions, where, minimum, maximum, abs, sqrt, erf, erfc): the
condition algebra and its folding, the definition errors, every operation's reverse mode and each function of
EveryPiecewiseOperation against torch.autograd in float64 (both branches, ties placed exactly, the NaN rules), the generated
text, and compilation for gfx950 (scratch and VGPRs of every fixed-grid kernel of the three test models)."""
import hashlib
import json
import math
import os
import re
import shutil

import pytest
import torch

from vihds import modelgen as G

import modelgen_models as MM
import modelgen_piecewise_models as PM
from test_modelgen_host import _check_vjp, _compile_usage, _define, _rand, _resource_usage
from test_modelgen_observe_host import _member

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64 = torch.float64
NAN, INF = float("nan"), float("inf")


# ---- tracing ----------------------------------------------------------------------------------------------------------------
def test_condition_algebra():
    g = G.Graph()
    a, b = g.leaf("th", 0), g.leaf("th", 1)
    lt, le = a < b, a <= b
    assert isinstance(lt, G.Cond) and lt.op == "lt" and le.op == "le" and lt.args == (a, b)
    # a > b is b < a, a >= b is b <= a; Python's reflected forms (number on the left) arrive the same way
    assert (b > a) is lt and (b >= a) is le
    assert (1.0 < a) is (a > 1.0) and (1.0 < a).args == (g.const(1.0), a)
    # repeated comparisons are one node (CSE), & and | are commutative, ~~c is c, c & c is c
    assert (a < b) is lt and len([n for n in g.nodes if n.op == "lt" and n.args[0] is a and n.args[1] is b]) == 1
    assert (lt & le) is (le & lt) and (lt | le) is (le | lt) and (lt & le).op == "and" and (lt | le).op == "or"
    assert (~lt).op == "not" and ~~lt is lt and (lt & lt) is lt and (lt | lt) is lt
    # ~(a < b) is not (a >= b): a NaN makes both comparisons false
    assert ~lt is not (a >= b)
    # Python bools combine: they decide or drop out
    assert (lt & True) is lt and (True & lt) is lt and (lt | False) is lt
    assert (lt & False).op == "cconst" and (lt & False).val is False and (lt | True).val is True


def test_folding_and_simplification():
    g = G.Graph()
    a, b = g.leaf("th", 0), g.leaf("th", 1)
    zero = a * 0.0  # (a constant node)
    assert zero.op == "const"
    c = zero < 1.0
    assert isinstance(c, G.Cond) and c.op == "cconst" and c.val is True and (~c).val is False
    assert (zero >= 1.0).val is False and (g.const(NAN) < 1.0).val is False and (g.const(NAN) >= 1.0).val is False
    # a constant condition selects when the model is traced; so does a Python bool
    assert G.where(c, a, b) is a and G.where(~c, a, b) is b and G.where(True, a, b) is a and G.where(False, a, 2.0).val == 2.0
    assert G.where(a < b, a, a) is a and G.where(a < b, 1.5, 1.5).val == 1.5
    w = G.where(a < b, a, b)
    assert w.op == "where" and G.where(b > a, a, b) is w
    # constant operands fold in float64
    val = lambda n: (n.op, n.val)  # noqa: E731
    assert val(G.minimum(zero, 2.0)) == ("const", 0.0) and val(G.maximum(zero, 2.0)) == ("const", 2.0)
    assert val(abs(zero - 3.0)) == ("const", 3.0) and val(G.sqrt(zero + 4.0)) == ("const", 2.0)
    assert val(G.erf(zero + 0.5)) == ("const", math.erf(0.5)) and val(G.erfc(zero + 0.5)) == ("const", math.erfc(0.5))
    assert math.isnan(G.minimum(zero + NAN, 1.0).val) and math.isnan(G.maximum(1.0, zero + NAN).val)
    assert math.isnan(G.sqrt(zero - 1.0).val)
    assert G.minimum(a, a) is a and G.maximum(a, a) is a
    # Python's abs() is the operation
    assert abs(a) is G.abs(a) and abs(a).op == "abs"
    # numbers and tensors dispatch as the other operations do
    assert G.minimum(1.0, 2.0) == 1.0 and G.maximum(1.0, 2.0) == 2.0 and G.abs(-2.0) == 2.0 and G.sqrt(4.0) == 2.0
    assert G.erf(0.5) == math.erf(0.5) and G.erfc(0.5) == math.erfc(0.5) and G.where(True, 1.0, 2.0) == 1.0
    assert math.isnan(G.minimum(NAN, 1.0)) and math.isnan(G.maximum(1.0, NAN)) and math.isnan(G.sqrt(-1.0))
    for name in ("where", "minimum", "maximum", "abs", "sqrt", "erf", "erfc"):
        assert name in G.OPERATIONS and getattr(G.op, name) is getattr(G, name)


def test_torch_dispatch_and_dtypes():
    for dtype in (torch.float64, torch.float32):
        x = torch.tensor([-1.5, 0.0, 0.5, 2.0], dtype=dtype)
        y = torch.tensor([1.0, 0.0, -0.5, 3.0], dtype=dtype)
        assert torch.equal(G.where(x < y, x, y), torch.where(x < y, x, y))
        assert torch.equal(G.where((x < y) & ~(x >= 0.0) | (y > 2.5), x, 0.25), torch.where((x < y) & ~(x >= 0) | (y > 2.5), x, y * 0 + 0.25))
        assert G.where(x < y, 0.1, x).dtype == dtype and G.where(x < y, x, 0.1).dtype == dtype
        assert torch.equal(G.minimum(x, y), torch.minimum(x, y)) and torch.equal(G.maximum(x, 0.25), torch.clamp_min(x, 0.25))
        assert G.minimum(0.1, x).dtype == dtype
        assert torch.equal(G.abs(x), x.abs()) and torch.equal(abs(x), x.abs())
        assert torch.equal(G.erf(x), torch.erf(x)) and torch.equal(G.erfc(x), torch.erfc(x))
        assert torch.equal(G.sqrt(y), torch.sqrt(y), ) or bool(torch.isnan(G.sqrt(y)[2]))
        # two numbers: 0 / 1 of a switch stay float32, which the tensors they meet promote; other numbers keep float64
        sel = G.where(x < y, 0.0, 1.0)
        assert sel.dtype == torch.float32 and (sel * x).dtype == dtype and sel.tolist() == [0.0, 1.0, 1.0, 0.0]
        assert G.where(x < y, 0.1, 0.2).dtype == torch.float64 and G.where(x < y, 0.1, 0.2)[0].item() == 0.1
    with pytest.raises(G.ModelDefinitionError, match="where"):
        G.where(torch.tensor([1.0]), 1.0, 2.0)


# ---- errors -----------------------------------------------------------------------------------------------------------------
def test_definition_errors():
    g = G.Graph()
    a, b = g.leaf("th", 0), g.leaf("th", 1)
    c = a < b
    for bad in (lambda: c + 1.0, lambda: 2.0 * c, lambda: -c, lambda: c / a, lambda: G.exp(c), lambda: G.where(c, c, a),
                lambda: G.minimum(c, a), lambda: c < a, lambda: abs(c)):
        with pytest.raises(G.ModelDefinitionError, match="arithmetic on a condition"):
            bad()
    with pytest.raises(G.ModelDefinitionError, match=r"where\(cond, a, b\).*not a model quantity"):
        G.where(a, a, b)
    with pytest.raises(G.ModelDefinitionError, match=r"where\(cond, a, b\).*not float"):
        G.where(1.0, a, b)
    with pytest.raises(G.ModelDefinitionError, match="& takes conditions"):
        c & a
    with pytest.raises(G.ModelDefinitionError, match="~ takes conditions"):
        ~a
    for bad in (lambda: a == b, lambda: a != 1.0, lambda: c == c):
        with pytest.raises(G.ModelDefinitionError, match="== and !="):
            bad()
    for bad in (lambda: bool(c), lambda: c and c, lambda: not c, lambda: 1.0 if a < b else 2.0):
        with pytest.raises(G.ModelDefinitionError, match="control flow.*where.*& | ~"):
            bad()

    def branchy(self, t, y, p, c):
        if y[0] > 1.0:
            return [y[0]] * 6
        return [p.r] * 6

    with pytest.raises(G.ModelDefinitionError, match="control flow"):
        _define("pw_bad_if", rhs=branchy)
    with pytest.raises(G.ModelDefinitionError, match="arithmetic on a condition"):
        _define("pw_bad_sum", rhs=lambda self, t, y, p, c: [(y[0] > 1.0) * p.r] + [0.0] * 5)
    with pytest.raises(G.ModelDefinitionError, match="arithmetic on a condition"):
        _define("pw_bad_return", rhs=lambda self, t, y, p, c: [y[0] > 1.0] + [0.0] * 5)
    # the initial state stays affine in theta with constant coefficients: init_vjp sees neither theta nor the treatments
    for k, init in enumerate((lambda th: G.where(th.init_x > 0.5, th.init_x, 0.5), lambda th: G.maximum(th.init_x, th.r),
                              lambda th: G.abs(th.init_x), lambda th: G.sqrt(th.init_x), lambda th: G.erf(th.init_x))):
        with pytest.raises(G.ModelDefinitionError, match="affine.*where, minimum, maximum"):
            _define("pw_bad_init%d" % k, initial_state=lambda self, th, c, f=init: [f(th), 0.0, 0.0, 0.0, 0.0, 0.0])
    # ... which a constant condition does not break
    assert _define("pw_ok_init", initial_state=lambda self, th, c: [G.where(True, th.init_x, 2.0 * th.init_x)] + [0.0] * 5)


# ---- adjoints ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,fn,n_args", [
    ("where", lambda a, b: G.where(a < b, a * b, a - b), 2),
    ("where_numbers", lambda a, b: b * G.where(a < 1.0, 0.0, 1.0) + G.where(a >= b, 0.5, a), 2),
    ("where_logic", lambda a, b, c: G.where((a < b) & ~(c <= 1.0) | (b > 1.5), a * c, G.exp(b)), 3),
    ("where_nested", lambda a, b, c: G.where(a < b, G.where(c > 1.0, a, b * c), G.where(c > a, c, 2.0)), 3),
    ("where_unselected_is_not_finite", lambda a, b: G.where(a < 3.0, a, G.log(a - 3.0)) * b, 2),  # (log of a negative: NaN)
    ("where_double", lambda a: G.where(a > 1.0, G.log(G.where(a > 1.0, a - 1.0, 1.0)), 0.0), 1),
    ("minimum", lambda a, b: G.minimum(a, b) * a, 2),
    ("maximum", lambda a, b: G.maximum(a, b) * b, 2),
    ("minimum_number", lambda a: G.minimum(a, 1.0) + G.maximum(0.7, a), 1),
    ("clamp_by_composition", lambda a, lo, hi: G.minimum(G.maximum(a, 0.5 * lo), 1.5 * hi), 3),
    ("abs", lambda a: G.abs(a - 1.0) * a, 1),
    ("abs_builtin", lambda a, b: abs(a - b), 2),
    ("sqrt", lambda a: G.sqrt(a) * a, 1),
    ("erf", lambda a: G.erf(a - 1.0), 1),
    ("erfc", lambda a: G.log(0.5 * G.erfc((a - 1.0) * 0.7)), 1),
    ("shot_noise", lambda s0, s1, x: 1.0 / (s0 * s0 + s1 * s1 * G.abs(x - 1.0)), 3),
])
def test_operation_vjp_matches_autograd(name, fn, n_args):
    xs = [_rand(seed=7 * k + 1) for k in range(n_args)]
    _check_vjp(fn, xs)


def _adjoints(fn, xs):
    g = G.Graph()
    leaves = [g.leaf("th", k) for k in range(len(xs))]
    out = fn(*leaves)
    adj = G.vjp(g, [out], [1.0])
    vals = G.evaluate([out] + [adj.get(l.id, g.const(0.0)) for l in leaves], {("th", k): x for k, x in enumerate(xs)})
    return vals[0], [v.expand_as(xs[0]) for v in vals[1:]]


def test_minimum_and_maximum_at_exact_ties():
    """g to the selected argument, g / 2 to each where the two are equal -- torch's rule."""
    a = torch.tensor([0.5, 1.0, 1.5, -2.0, 0.0], dtype=F64)
    b = torch.tensor([1.0, 1.0, 1.0, -2.0, -0.0], dtype=F64)
    for fn in (G.minimum, G.maximum):
        _check_vjp(fn, [a, b])
        _check_vjp(lambda x, f=fn: f(x, 1.0), [a])
    _, (da, db) = _adjoints(G.minimum, [a, b])
    assert da.tolist() == [1.0, 0.5, 0.0, 0.5, 0.5] and db.tolist() == [0.0, 0.5, 1.0, 0.5, 0.5]
    _, (da, db) = _adjoints(G.maximum, [a, b])
    assert da.tolist() == [0.0, 0.5, 1.0, 0.5, 0.5] and db.tolist() == [1.0, 0.5, 0.0, 0.5, 0.5]


def test_abs_and_sqrt_at_zero():
    x = torch.tensor([-1.5, 0.0, 2.0], dtype=F64)
    _check_vjp(lambda a: G.abs(a), [x])
    _, (d,) = _adjoints(G.abs, [x])
    assert d.tolist() == [-1.0, 0.0, 1.0]
    v, (d,) = _adjoints(G.sqrt, [torch.tensor([0.0, 4.0], dtype=F64)])
    assert v.tolist() == [0.0, 2.0] and d.tolist() == [INF, 0.25]  # (infinite at 0, as torch's)


def test_where_adjoint_is_a_select_not_a_product():
    """The branch not taken may hold anything: its adjoint is 0, not 0 * inf."""
    x = torch.tensor([0.0, 0.5, 2.0], dtype=F64)
    fn = lambda a: G.where(a > 1.0, a * a, 1.0 / a)  # noqa: E731  (1 / 0 = inf at the first element, whose branch is taken)
    v, (d,) = _adjoints(fn, [x])
    assert v.tolist() == [INF, 2.0, 4.0] and d[1:].tolist() == [-4.0, 4.0]
    # what the select does not do is repair the branch not taken: sqrt of a negative there is NaN, and 0 / NaN stays NaN --
    # exactly as torch.where's backward leaves it (the double-where idiom of the module docstring is the cure)
    fn = lambda a: G.where(a < 1.0, a, G.sqrt(a - 1.0))  # noqa: E731
    v, (d,) = _adjoints(fn, [x])
    xt = x.clone().requires_grad_(True)
    (ref,) = torch.autograd.grad(fn(xt).sum(), xt)
    assert v.tolist() == [0.0, 0.5, 1.0] and torch.isnan(d).tolist() == torch.isnan(ref).tolist() == [True, True, False]
    assert float(d[2]) == float(ref[2]) == 0.5
    safe = lambda a: G.where(a < 1.0, a, G.sqrt(G.where(a < 1.0, 1.0, a - 1.0)))  # noqa: E731
    v, (d,) = _adjoints(safe, [x])
    assert v.tolist() == [0.0, 0.5, 1.0] and d.tolist() == [1.0, 1.0, 0.5]
    # the seed of the branch not taken is exactly zero, so a finite local derivative there contributes nothing
    g = G.Graph()
    a, seed = g.leaf("th", 0), g.leaf("seed", 0)
    adj = G.vjp(g, [G.where(a > 1.0, a * 3.0, a)], [seed])[a.id]
    ops_used = {n.op for n in G._topo([adj])}
    assert "where" in ops_used and not ops_used & {"cpass", "minpass", "maxpass", "sign"}


def test_nan_semantics_are_torchs():
    """A NaN operand makes every comparison false; minimum / maximum return the NaN (fminf / fmaxf would return the other
    argument); a NaN stays one through where, abs, sqrt, erf and erfc."""
    a = torch.tensor([NAN, 1.0, NAN, 2.0], dtype=F64)
    b = torch.tensor([1.0, NAN, NAN, 1.0], dtype=F64)
    g = G.Graph()
    x, y = g.leaf("th", 0), g.leaf("th", 1)
    env = {("th", 0): a, ("th", 1): b}
    nodes = [G.where(x < y, 1.0, 0.0), G.where(x <= y, 1.0, 0.0), G.where(x > y, 1.0, 0.0), G.where(x >= y, 1.0, 0.0),
             G.where(~(x < y), 1.0, 0.0), G.minimum(x, y), G.maximum(x, y), G.maximum(x, 0.5), G.minimum(0.5, y),
             G.abs(x), G.sqrt(x), G.erf(x), G.erfc(x), G.where(y > 0.0, x, y)]
    lt, le, gt, ge, nlt, mn, mx, mx_c, mn_c, ab, sq, ef, efc, wh = G.evaluate(nodes, env)
    assert lt.tolist() == [0, 0, 0, 0] and le.tolist() == [0, 0, 0, 0] and gt.tolist() == [0, 0, 0, 1]
    assert ge.tolist() == [0, 0, 0, 1] and nlt.tolist() == [1, 1, 1, 1]
    same = lambda u, v: torch.equal(torch.isnan(u), torch.isnan(v)) and torch.equal(u.nan_to_num(7.0), v.nan_to_num(7.0))  # noqa: E731
    assert same(mn, torch.minimum(a, b)) and same(mx, torch.maximum(a, b)) and torch.isnan(mn).tolist() == [1, 1, 1, 0]
    assert torch.isnan(mx_c).tolist() == [1, 0, 1, 0] and torch.isnan(mn_c).tolist() == [0, 1, 1, 0]
    for v in (ab, sq, ef, efc):
        assert torch.isnan(v).tolist() == [1, 0, 1, 0]
    assert torch.isnan(wh).tolist() == [1, 1, 1, 0]
    # the torch dispatch of the same expressions is torch itself; constants fold the same way
    assert same(G.minimum(a, b), mn) and same(G.maximum(a, 0.5), mx_c)
    z = x * 0.0
    assert math.isnan(G.maximum(z + NAN, 0.5).val) and math.isnan(G.minimum(0.5, z + NAN).val) and G.where(z + NAN < 1.0, 1.0, 2.0).val == 2.0


def _function_case(which, n=400, seed=3):
    """One of the five functions of EveryPiecewiseOperation: its traced outputs, the DAG leaves it reads with random float64
    values, and the same method called on those values as tensors (the torch dispatch)."""
    cls = PM.EveryPiecewiseOperation
    tr, g = cls._trace, cls._trace.g
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda lo, hi: lo + (hi - lo) * torch.rand(n, dtype=F64, generator=gen)  # noqa: E731
    inst = cls.__new__(cls)
    NPU, P = len(tr.p_names), cls.parameter_names
    c0 = rnd(0.2, 2.0)
    if which == "prepare":
        vals = {n_: PM.EVERY_BASE[n_] * rnd(0.5, 1.6) for n_ in P}
        vals["K"] = vals["K"] * torch.where(rnd(0, 1) < 0.3, -1.0, 1.0)  # (abs: both signs)
        leaves = {("th", s): vals[n_] for s, n_ in enumerate(P)}
        leaves[("c", 0)] = c0
        outs = tr.p_exprs

        def call(v):
            th = G._Named([(n_, v[("th", s)]) for s, n_ in enumerate(P)], "parameter")
            return list(inst.prepare(th, G._Conditions([v[("c", 0)]])).values())
        return outs, leaves, call, [("c", 0)]
    pv = {k: PM.EVERY_BASE[name] * rnd(0.5, 1.6) for k, name in enumerate(tr.p_names)}
    pv[tr.p_names.index("tau")] = rnd(0.4, 4.6)
    leaves = {("p", k): v for k, v in pv.items()}
    leaves[("p", NPU)] = c0
    named = lambda v: G._Named([(name, v[("p", k)]) for k, name in enumerate(tr.p_names)], "effective parameter")  # noqa: E731
    cs = lambda v: G._Conditions([v[("p", NPU)]])  # noqa: E731
    ys = lambda v: [v[("y", j)] for j in range(4)]  # noqa: E731
    xs = lambda v: [v[("x", j)] for j in range(4)]  # noqa: E731
    no_grad = [("p", NPU)]
    if which in ("rhs", "observe", "precision"):
        leaves.update({("y", j): rnd(0.05, 2.0) for j in range(4)})
    if which == "rhs":
        leaves[("t", 0)] = rnd(0.0, 4.0)
        no_grad.append(("t", 0))
        return tr.dy, leaves, lambda v: inst.rhs(v[("t", 0)], ys(v), named(v), cs(v)), no_grad
    if which == "observe":
        return tr.obs, leaves, lambda v: cls._observe_def(inst, ys(v), named(v), cs(v)), no_grad
    leaves.update({("x", j): rnd(0.05, 2.0) for j in range(4)})
    if which == "precision":
        return tr.prec, leaves, lambda v: cls._precision_def(inst, ys(v), xs(v), named(v), cs(v)), no_grad
    leaves.update({("ob", j): rnd(0.05, 2.5) for j in range(4)})
    leaves.update({("pr", j): rnd(5.0, 50.0) for j in range(4)})
    no_grad += [("ob", j) for j in range(4)]
    return (tr.lik, leaves,
            lambda v: cls._likelihood_def(inst, xs(v), [v[("ob", j)] for j in range(4)], [v[("pr", j)] for j in range(4)], named(v), cs(v)),
            no_grad)


@pytest.mark.parametrize("which", ["prepare", "rhs", "observe", "precision", "log_likelihood"])
def test_every_function_of_the_model_against_autograd(which):
    """Reverse mode over the traced function, evaluated in float64, against torch.autograd through the same method on tensors
    (the torch dispatch): the values and the adjoint of every leaf within 1e-12; every switch of the function goes both ways
    on these inputs."""
    outs, leaves, call, no_grad = _function_case(which)
    g = PM.EveryPiecewiseOperation._trace.g
    gen = torch.Generator().manual_seed(9)
    n = next(iter(leaves.values())).shape[0]
    W = [torch.randn(n, dtype=F64, generator=gen) for _ in outs]
    adj = G.vjp(g, outs, [g.leaf("seed", k) for k in range(len(outs))])
    keys = [k for k in leaves if k not in no_grad]
    env = dict(leaves)
    env.update({("seed", k): w for k, w in enumerate(W)})
    vals = G.evaluate(list(outs) + [adj.get(g.leaf(*k).id, g.const(0.0)) for k in keys], env)
    tens = {k: (v.clone().requires_grad_(True) if k in keys else v) for k, v in leaves.items()}
    with PM.recording() as m:
        ref = call(tens)
    ref = [r if isinstance(r, torch.Tensor) else torch.full((n,), float(r), dtype=F64) for r in ref]
    err = lambda a, b: ((a - b).abs() / (1.0 + b.abs())).max().item()  # noqa: E731
    for k, (a, b) in enumerate(zip(vals[:len(outs)], ref)):
        assert bool(torch.isfinite(b).all()) and err(a.expand(n), b) <= 1e-12, (which, k)
    total = sum((r * w).sum() for r, w in zip(ref, W) if r.requires_grad)
    grads = torch.autograd.grad(total, [tens[k] for k in keys], allow_unused=True)
    nonzero = 0
    for k, a, b in zip(keys, vals[len(outs):], grads):
        b = torch.zeros(n, dtype=F64) if b is None else b
        assert bool(torch.isfinite(b).all()) and err(a.expand(n), b) <= 1e-12, (which, k)
        nonzero += int(bool((b != 0).any()))
    assert nonzero >= 4 and m.by_label, which
    # both sides of every switch whose sides these inputs can reach: the recorded margins say where each was evaluated; the
    # selects themselves are read off the outputs
    cls = PM.EveryPiecewiseOperation
    tr = cls._trace
    if which == "rhs":
        t, tau = leaves[("t", 0)], leaves[("p", tr.p_names.index("tau"))]
        x, thr = leaves[("y", 0)], leaves[("p", tr.p_names.index("thr"))]
        boost_grad = grads[keys.index(("p", tr.p_names.index("boost")))]
        taken = (t >= tau) & (x > thr)
        assert bool(taken.any()) and bool((~taken).any())
        assert bool((boost_grad[taken] != 0).all()) and bool((boost_grad[~taken] == 0).all())  # (read in one branch only)
    if which == "log_likelihood":
        censored = leaves[("ob", 1)] >= leaves[("p", tr.p_names.index("ceil"))]
        assert bool(censored.any()) and bool((~censored).any())


def test_tobit_far_below_the_ceiling_has_a_finite_adjoint():
    """The trap the module docstring describes: a dozen standard deviations below the ceiling erfc underflows in float32, and
    log's adjoint in the branch not taken is 0 / 0 unless the argument is made safe by an inner where (PM._tobit does)."""
    x = torch.tensor([0.1, 2.9], dtype=torch.float32, requires_grad=True)
    ob, pr, ceil = torch.tensor([0.1, 3.0]), torch.tensor([1e4, 1e4]), torch.tensor([3.0, 3.0])
    ll = PM._tobit(x, ob, pr, ceil, "test")
    ll.sum().backward()
    assert bool(torch.isfinite(ll).all()) and bool(torch.isfinite(x.grad).all()) and float(x.grad[1]) > 0.0
    xn = x.detach().clone().requires_grad_(True)
    naive = G.where(ob >= ceil, G.log(0.5 * G.erfc((ceil - xn) * G.sqrt(pr) * PM.SQRT1_2)), -0.5 * pr * (xn - ob) * (xn - ob))
    naive.sum().backward()
    assert bool(torch.isfinite(naive).all()) and not bool(torch.isfinite(xn.grad).all())


# ---- generated text ---------------------------------------------------------------------------------------------------------
TIME_LOOP = ["rhs", "rhs_vjp", "observe", "observe_vjp", "precision", "precision_vjp", "loglik", "loglik_vjp"]


def test_generated_text():
    cls = PM.EveryPiecewiseOperation
    src = G.generate_source(cls)
    assert src == G.generate_source(cls)
    for c, neural in PM.PREBUILT:
        text = G.generate_source(c, neural)
        assert "if (" not in text and "?" not in text and "fmaxf" not in text and "fminf" not in text, c.__name__
    loop = "\n".join(_member(src, m) for m in TIME_LOOP)
    once = "\n".join(_member(src, m) for m in ("prepare", "prepare_vjp", "init", "init_vjp"))
    # the time loop uses the helpers of vihds_models.hpp, prepare the accurate forms
    for form in ("fsel(", "fmin_nan(", "fmax_nan(", "min_pass(", "max_pass(", "fsign(", "fabsf(", "fsqrt(", "erff(", "erfcf(",
                 " < ", " <= ", " && ", " || ", "const bool v", "!v"):
        assert form in loop, form
    for form in ("sqrtf(", "expf(", " / ", "tanhf("):
        assert form not in loop, form
    for form in ("sqrtf(", "fabsf(", "fsign(", "erff(", "erfcf(", "fsel(", "fmin_nan(", "fmax_nan(", "expf("):
        assert form in once, form
    assert "fsqrt(" not in once and "fexp(" not in once
    # where's adjoint is a select of the seed: no product with a mask.  In rhs_vjp every multiplication by a pass weight
    # belongs to minimum / maximum / abs
    body = _member(src, "rhs_vjp")
    assert re.search(r"const float v\d+ = fsel\(v\d+, 0\.0f, v\d+\);", body) or re.search(r"fsel\(v\d+, v\d+, 0\.0f\)", body)
    tr = cls._trace
    k_boost = tr.p_names.index("boost")
    written = sorted(int(k) for k in re.findall(r"pb\[(\d+)\] \+=", body))
    assert k_boost in written  # (the parameter that one where branch reads)
    m = re.search(r"pb\[%d\] \+= (v\d+);" % k_boost, body)
    expr = re.search(r"const float %s = (.*);" % m.group(1), body).group(1)
    operands = [re.search(r"const (?:float|bool) %s = (.*);" % v, body).group(1) for v in re.findall(r"v\d+", expr)]
    assert any(o.startswith("fsel(") for o in operands), (expr, operands)  # (y[0] times a SELECTED seed)
    assert not any("_pass(" in o or "fsign(" in o for o in operands), (expr, operands)
    # conditions are shared: one comparison of t with tau in rhs, one in its adjoint
    tau = "p[%d]" % tr.p_names.index("tau")
    assert len(re.findall(r"const bool v\d+ = t < %s;" % re.escape(tau), _member(src, "rhs"))) == 1
    assert len(re.findall(r"const bool v\d+ = t < %s;" % re.escape(tau), body)) == 1
    # PrprDosed: the treatment is a parameter behind the named ones, compared with t; it has no adjoint
    dosed = G.generate_source(PM.PrprDosed)
    npu = len(PM.PrprDosed._trace.p_names)
    assert "    p[%d] = c[0];" % npu in _member(dosed, "prepare") and "t < p[%d]" % npu in _member(dosed, "rhs")
    assert "pb[%d]" % npu not in _member(dosed, "rhs_vjp")


def test_recorded_digests_of_the_existing_models_are_unchanged():
    with open(os.path.join(ROOT, "tests", "golden", "modelgen_source_sha256.json")) as f:
        recorded = json.load(f)
    assert len(recorded) == 12
    for key, digest in recorded.items():
        name, neural = key.split(":")
        text = G.generate_source(getattr(MM, name), bool(int(neural)))
        assert hashlib.sha256(text.encode()).hexdigest() == digest, key


def test_docstring_names_the_operations_and_the_traps():
    doc = G.__doc__
    for word in ("where(", "minimum", "maximum", "abs", "sqrt", "erf", "erfc", "& | ~", "double-where", "switch time",
                 "minimum(maximum(x, lo), hi)"):
        assert word in doc, word


# ---- the inputs of the GPU tests ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", [PM.EveryPiecewiseOperation, PM.PrprDosed], ids=lambda c: c.__name__)
def test_the_float64_yardstick_keeps_every_switch_wide(cls):
    """The precondition of the GPU comparisons, on the yardstick alone (B=3, S=5): the smallest margin of every switch over
    every stage of every fixed-grid solver is at least 1e-3, and both sides of the model's switches occur."""
    pb = PM.problem(cls, 3, 5)
    for solver in PM.FIXED:
        with PM.recording() as m:
            xs, xp, prec, logp = PM.forward(cls, pb["th"], pb["cond"], pb["times"], solver, pb["obs"])
        print("%s %s: smallest margin %.2e (%s)" % (cls.__name__, solver, m.smallest, min(m.by_label, key=m.by_label.get)))
        assert m.smallest >= PM.MARGIN and bool(torch.isfinite(logp).all())
    if cls is PM.EveryPiecewiseOperation:
        assert bool((pb["th"]["tau"] > pb["times"][-1]).any()) and bool((pb["th"]["tau"] < 3.0).any())
        censored = pb["obs"][:, None, 1] >= pb["th"]["ceil"][:, :, None]
        assert bool(censored.any()) and bool((~censored).any())


# ---- compilation --------------------------------------------------------------------------------------------------------------
SOLVERS = ["MODEULER", "MODEULERWHILE", "EULER", "MIDPOINT", "RK4"]


@pytest.mark.skipif(not (shutil.which("hipcc") or os.path.exists("/opt/rocm/bin/hipcc")), reason="hipcc not installed")
@pytest.mark.parametrize("cls", [c for c, _ in PM.PREBUILT], ids=lambda c: c.__name__)
def test_piecewise_models_compile_without_scratch_for_every_fixed_grid_solver(tmp_path, cls):
    """Forward and adjoint kernels of the three models for every fixed-grid solver: they compile for gfx950 and spill
    nothing.  (VGPR ranges printed, recorded in DESIGN.md section 4.)"""
    header = tmp_path / "piecewise.hpp"
    header.write_text(G.generate_source(cls))
    lines = ['#include "vihds_ode_kernels.hpp"', '#include "%s"' % header, "namespace vihds {"]
    for s in SOLVERS:
        lines.append("template __global__ void ode_fwd_kernel<VIHDS_GEN_CORE, VIHDS_SOLVER_%s, true>(OdeArgs);" % s)
        lines.append("template __global__ void ode_bwd_kernel<VIHDS_GEN_CORE, VIHDS_SOLVER_%s, false>(OdeArgs);" % s)
    lines.append("}")
    usage = _resource_usage(_compile_usage(tmp_path, "\n".join(lines) + "\n", "piecewise"), "_ZN5vihds")
    assert len(usage) == 2 * len(SOLVERS), sorted(usage)
    for kind in ("ode_fwd_kernel", "ode_bwd_kernel"):
        vgprs = [v for name, (v, _) in usage.items() if kind in name]
        print("%s %s: %d .. %d VGPRs" % (cls.__name__, kind, min(vgprs), max(vgprs)))
    for name, (vgpr, scratch) in sorted(usage.items()):
        assert scratch == 0, name
