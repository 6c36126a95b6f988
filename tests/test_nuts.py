"""CPU tests of the no-U-turn sampler: the restated transition (``tests/nuts_ref.py``) against
an independently written recursive NUTS, its stationarity at exact levels with a power table of
mutants, dual averaging, and the C ABI's new entry points (symbols, signatures, refusals)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import nuts_ref as N
import stationarity as S
from binf_amd import _native
from conftest import ROOT

f64 = np.float64


# ---------------------------------------------------------------------------
# checkpoint ranges
# ---------------------------------------------------------------------------
def _aligned_subtrees_ending_at(n, lo=0, size=1 << 12):
    """Sizes (> 1) of the nodes of a perfect binary tree over leaves [lo, lo + size) whose last
    leaf is ``n``, by recursion over the tree."""
    if size == 1:
        return []
    half = size // 2
    out = [size] if lo + size - 1 == n else []
    return out + (_aligned_subtrees_ending_at(n, lo, half) if n < lo + half
                  else _aligned_subtrees_ending_at(n, lo + half, half))


def test_checkpoint_ranges_cover_exactly_the_aligned_subtrees_that_end_at_a_leaf():
    """Walking the leaves 0 ... 2^12 - 1 in order and storing every even leaf at level ``hi``:
    the levels ``lo ... hi`` of an odd leaf hold exactly the FIRST leaves of the aligned sub-trees
    that end at it (sizes 2, 4, ... largest at ``lo``), still unoverwritten."""
    stored = {}
    for n in range(1 << 12):
        lo, hi = N.checkpoint_range(n)
        if n % 2 == 0:
            assert lo == hi + 1 and 0 <= hi < 12
            stored[hi] = n
            assert _aligned_subtrees_ending_at(n) == []
            continue
        want = sorted(_aligned_subtrees_ending_at(n))            # 2, 4, ..., 2^k
        assert want == [2 << t for t in range(len(want))] and len(want) == hi - lo + 1
        assert lo >= 0
        for t, size in enumerate(want):
            assert stored[hi - t] == n - size + 1, (n, t)


# ---------------------------------------------------------------------------
# the same trees as a recursive NUTS
# ---------------------------------------------------------------------------
class _Recursive(object):
    """Multinomial NUTS by recursion for ONE chain, written from the textbook (Betancourt 2017,
    appendix A; Stan's transition): doubling in a random direction, U-turn checks at every node
    of the new sub-tree, uniform progressive sampling inside it (a running reservoir over its
    leaves), biased progressive sampling between the old tree and the new sub-tree."""

    def __init__(self, sigma, eps, md, max_delta, u):
        self.w2, self.eps, self.md, self.max_delta = 1.0 / (sigma * sigma), f64(eps), md, max_delta
        self.udir, self.umerge, self.uleaf = u[:md], u[md:2 * md], u[2 * md:]

    def grad(self, q):
        return q * self.w2

    def energy(self, q, r):
        return -(-0.5 * np.sum(q * (q * self.w2))) + f64(0.5) * np.sum(r * r)

    def step(self, s, v):
        q, r, g = s
        dt = f64(v) * self.eps
        r = r - (f64(0.5) * dt) * g
        q = q + r * dt
        g = self.grad(q)
        return q, r - (f64(0.5) * dt) * g, g

    def build(self, s, v, depth):
        """Extends from ``s`` by 2^depth leaves; returns (last state, first r, last r, rho, ok)."""
        if depth == 0:
            s = self.step(s, v)
            self.leaves.append(s[0].copy())
            k = len(self.leaves) - 1
            delta = self.energy(s[0], s[1]) - self.H0
            if not delta <= self.max_delta:
                self.end = 'DIV'
                return s, s[1], s[1], s[1], False
            w = np.exp(-delta)
            self.w_sub += w
            if self.uleaf[k] * self.w_sub < w:
                self.cand = s[0]
            return s, s[1], s[1], s[1].copy(), True
        s, a_first, a_last, a_rho, ok = self.build(s, v, depth - 1)
        if not ok:
            return s, None, None, None, False
        s, b_first, b_last, b_rho, ok = self.build(s, v, depth - 1)
        if not ok:
            return s, None, None, None, False
        rho = a_rho + b_rho
        if np.sum(a_first * rho) <= 0.0 or np.sum(b_last * rho) <= 0.0:
            self.end = 'SUBTURN'
            return s, None, None, None, False
        return s, a_first, b_last, rho, True

    def run(self, q0, r0):
        s0 = (q0, r0, self.grad(q0))
        self.H0 = self.energy(q0, r0)
        self.leaves, self.end = [], None
        edge = {1: s0, -1: s0}
        prop, w_tree, rho_tree, depth = q0, 1.0, r0.copy(), 0
        while True:
            v = 1 if self.udir[depth] < 0.5 else -1
            self.w_sub, self.cand = 0.0, None
            s, _, _, rho, ok = self.build(edge[v], v, depth)
            if not ok:
                return prop, self.end, depth
            if self.umerge[depth] * w_tree < self.w_sub:
                prop = self.cand
            w_tree += self.w_sub
            rho_tree = rho_tree + rho
            edge[v] = s
            depth += 1
            if np.sum(edge[-1][1] * rho_tree) <= 0.0 or np.sum(edge[1][1] * rho_tree) <= 0.0:
                return prop, 'TURN', depth
            if depth == self.md:
                return prop, 'MAXD', depth


@pytest.mark.parametrize('D', [1, 3, 8])
def test_restated_transition_builds_the_trees_of_a_recursive_nuts(D):
    """500 random (q0, r0, u), max_depth 5: the same leaves in the same order, the same
    termination and depth, the same proposal, chain by chain.  (The recursion sums rho and the
    weights in tree order and without the running reference energy, so a selection or a U-turn
    dot within rounding of its threshold could differ: none of these draws is that close.)"""
    C, md = 500, 5
    rs = np.random.RandomState(100 + D)
    sigma = np.exp(rs.uniform(-1.0, 1.0, size=D))
    q0 = sigma * rs.standard_normal((C, D))
    q0[::50] *= 40.0                                           # some chains far out ...
    r0 = rs.standard_normal((C, D))
    u = rs.uniform(size=(C, N.n_uniforms(md)))
    eps = np.exp(rs.uniform(np.log(0.05), np.log(1.9), size=C)) * sigma.min()
    eps[::50] = 2.5 * sigma.min()                              # ... with a step that diverges there
    grad = lambda q: q * (1.0 / (sigma * sigma))
    logp = lambda q: -0.5 * np.sum(q * grad(q), axis=1)
    tree = N.Tree(C, D, md, max_delta=1000.0)
    out = N.transition(tree, N.Integrator(), logp, grad, q0, r0, eps, u, track=True)
    names = {N.TURN: 'TURN', N.SUBTURN: 'SUBTURN', N.MAXD: 'MAXD', N.DIV: 'DIV'}
    seen = set()
    for c in range(C):
        rec = _Recursive(sigma, eps[c], md, 1000.0, u[c])
        prop, end, depth = rec.run(q0[c], r0[c])
        seen.add(end)
        assert end == names[int(tree.status[c])], c
        assert depth == tree.tree_depth[c], c
        assert len(rec.leaves) == tree.n_leap[c] == len(tree.visited[c]), c
        assert all(np.array_equal(a, b) for a, b in zip(rec.leaves, tree.visited[c])), c
        assert np.array_equal(prop, out[c]), c
        assert bool(tree.moved[c]) == (not np.array_equal(out[c], q0[c])), c
    assert seen == set(names.values()), seen


def test_rowdot_is_numpys_sum_of_a_contiguous_row():
    rs = np.random.RandomState(3)
    for D in (1, 7, 129, 1000, 8192):
        a, b = rs.standard_normal((5, D)), rs.standard_normal((5, D))
        assert np.array_equal(N.rowdot(a, b), np.array([np.sum(a[c] * b[c]) for c in range(5)]))


# ---------------------------------------------------------------------------
# stationarity and its power
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('kind', sorted(N.STATIONARITY))
def test_restated_sampler_keeps_the_target(kind):
    """sigma = (1, 2, 3, 5, 10), 4000 chains x 3 transitions from exact draws, identity /
    mismatched diagonal / mismatched dense metric (the dense one on the rotated target): pooled
    chi^2, pooled mean and DKW at the exact levels of ``tests/stationarity.py``."""
    case, x, tree = N.run_stationarity(kind)
    checks = N.stationarity_checks(case, x, N.stationarity_alpha())
    for c in checks:
        print(S.describe(c))
    assert all(S.inside(c) for c in checks), [S.describe(c) for c in checks]
    assert tree.n_divergent.sum() == 0


# measured at the stationarity runs' own size (4000 chains x 3 transitions, identity metric, seed 0),
# where the first mutant is in reach already, so the sizes were not grown: sound 0.05,
# no_subtree_check 3.20.  OUT OF REACH of the pooled chi^2 at this size, with their measured margins
# (at 40000 chains, measured once and not run here, they reach 3.1 and 3.4):
OUT_OF_REACH = {'cand_last_leaf': 0.93, 'edges_not_updated': 1.11}


def test_power_table_of_the_stationarity_statistics():
    """What the statistics above can see.  'No sub-tree check' must reach a pooled-chi^2 margin
    (|z| over the threshold's z) >= 2 where the sound sampler stays <= 1.  'Candidate always the
    last leaf' and 'edges not updated on merge' do not reach 2 at this size: they are listed in
    ``OUT_OF_REACH`` with their measured margins, not dropped -- the recursive-tree test above is
    what pins the candidate rule and the edges."""
    alpha = N.stationarity_alpha()
    got = {}
    for mutant in (None,) + N.MUTANTS:
        case, x, _ = N.run_stationarity('identity', seed=0, mutant=mutant)
        got[mutant] = S.chi2_margin(N.stationarity_checks(case, x, alpha))
        print('%-20s margin %.2f' % (mutant, got[mutant]))
    assert got[None] <= 1.0
    for mutant in N.MUTANTS:
        if mutant in OUT_OF_REACH:
            assert abs(got[mutant] - OUT_OF_REACH[mutant]) < 0.01, 'the listed margin is stale'
            assert got[mutant] < S.MARGIN, 'in reach after all: move it into the table'
        else:
            assert got[mutant] >= S.MARGIN, (mutant, got[mutant])


# ---------------------------------------------------------------------------
# dual averaging
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('seed', [0, 1, 2])
@pytest.mark.parametrize('eps0', [0.01, 5.0])
def test_dual_averaging_finds_the_step(seed, eps0):
    """sigma = (1, 2, 3, 5, 10), identity metric, starts 3 sigma out, max_depth 8: after 150
    adapting transitions the frozen steps lie in [0.9, 1.5] from eps = 0.01 and from eps = 5, and
    the mean accept_stat of the next 100 transitions in [0.75, 0.97]."""
    C, md = 16, 8
    case = N.Case('identity')
    rs = np.random.RandomState(seed)
    x = 3.0 * case.sigma * np.sign(rs.standard_normal((C, 5)))
    s = N.NUTS(case.logp, case.grad, x, eps0, md, adaption_limit=151)
    draw = lambda: (rs.standard_normal((C, 5)), rs.uniform(size=(C, N.n_uniforms(md))))
    for _ in range(150):
        s.sample(*draw())
    frozen = s.eps.copy()
    print('frozen steps %.3f ... %.3f' % (frozen.min(), frozen.max()))
    assert np.all((frozen >= 0.9) & (frozen <= 1.5)), frozen
    stat = []
    for _ in range(100):
        s.sample(*draw())
        stat.append(s.tree.accept_stat.copy())
    assert np.array_equal(s.eps, frozen)
    m = float(np.mean(stat))
    print('mean accept_stat %.3f' % m)
    assert 0.75 <= m <= 0.97, m


# ---------------------------------------------------------------------------
# C ABI
# ---------------------------------------------------------------------------
NEW_SYMBOLS = ('binf_nuts_begin_f64', 'binf_nuts_leaf_f64', 'binf_nuts_pending', 'binf_nuts_adapt_step_f64')


def test_new_symbols_are_declared_exported_and_bound_argument_by_argument():
    import test_native_abi as T
    protos = T.header_prototypes()
    raw = ctypes.CDLL(_native.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in protos and hasattr(raw, name) and name in _native.SIGNATURES, name
        ret, args = protos[name]
        res, bound = _native.SIGNATURES[name]
        assert res is T._ctype_of(ret) and len(bound) == len(args), name
        for c, b in zip(args, bound):
            want = T._ctype_of(c)
            assert T._is_pointer_binding(b) if want == 'pointer' else b is want, (name, c, b)
    assert protos['binf_nuts_adapt_step_f64'][1] == ['double*', 'const double*', 'double*', 'double*', 'double*',
                                                     'double*', 'double', 'double', 'double', 'double', 'int32_t',
                                                     'int64_t', 'void*']
    assert _native.lib().binf_abi_version() == 7


def test_nuts_args_layout_matches_the_header(tmp_path):
    fields = [f[0] for f in _native.NutsArgs._fields_]
    src = tmp_path / 'layout.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "binf_hip.h"\nint main(void) {\n'
                   '  printf("%zu\\n", sizeof(binf_nuts_args));\n' +
                   ''.join('  printf("%%zu\\n", offsetof(binf_nuts_args, %s));\n' % f for f in fields) +
                   '  return 0; }\n')
    exe = tmp_path / 'layout'
    subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    out = [int(x) for x in subprocess.check_output([str(exe)]).split()]
    assert out[0] == ctypes.sizeof(_native.NutsArgs)
    for f, off in zip(fields, out[1:]):
        assert getattr(_native.NutsArgs, f).offset == off, f
    hdr = open(os.path.join(ROOT, 'include', 'binf_hip.h')).read()
    body = hdr[hdr.index('typedef struct binf_nuts_args {'):hdr.index('} binf_nuts_args;')]
    import re
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    declared = []
    for stmt in body.split('{', 1)[1].split(';'):
        if stmt.strip():
            names = stmt.replace('*', ' ').split(',')
            declared.append(names[0].split()[-1])
            declared += [n.strip() for n in names[1:]]
    assert declared == fields


def _fake_args(C=4, D=16, md=3):
    """An argument block over addresses that are never dereferenced (refusals come first)."""
    a = _native.NutsArgs()
    a.struct_size = ctypes.sizeof(a)
    base = 1 << 40
    for i, name in enumerate(_native.NUTS_ROWS + _native.NUTS_F64 + _native.NUTS_I32 + _native.NUTS_U8 + _native.NUTS_I64):
        setattr(a, name, base + (i << 34))
    a.max_delta, a.C, a.D, a.max_depth, a.reserved = 1000.0, C, D, md, 0
    return a


@pytest.mark.parametrize('entry', ['binf_nuts_begin_f64', 'binf_nuts_leaf_f64'])
def test_refusals_come_before_any_launch(entry):
    """max_depth 0 / 13, D = 8193, a struct of another size, a NULL array and overlapping pairs:
    every one answered on the host (these addresses do not exist, and there is no GPU here)."""
    f = getattr(_native.lib(), entry)
    call = lambda a: f(ctypes.byref(a), None)
    for md in (0, 13, -1):
        assert call(_fake_args(md=md)) == _native.E_ARG and 'max_depth' in _native.last_error()
    assert call(_fake_args(D=8193)) == _native.E_UNSUPPORTED
    with pytest.raises(NotImplementedError):
        _native.check(call(_fake_args(D=8193)), entry)
    assert call(_fake_args(D=0)) == _native.E_ARG
    assert call(_fake_args(C=-1)) == _native.E_ARG
    a = _fake_args()
    a.struct_size -= 8
    assert call(a) == _native.E_ARG and 'struct_size' in _native.last_error()
    a = _fake_args()
    a.cand = None
    assert call(a) == _native.E_ARG and 'cand' in _native.last_error()
    C, D, md = 4, 16, 3
    for name, other, shift in (('q_out', 'prop', 8), ('q_out', 'prop', C * D * 8 - 8), ('r', 'q', 0),
                               ('ck_rho', 'ck_r', C * D * md * 8 - 8), ('edge_r', 'edge_q', 2 * C * D * 8 - 8),
                               ('dt_dir', 'eps', C * 8 - 8), ('status', 'n_leap', 4), ('diverging', 'moved', C - 1),
                               ('n_divergent', 'u', C * N.n_uniforms(md) * 8 - 8)):
        a = _fake_args(C, D, md)
        setattr(a, name, getattr(a, other) + shift)
        assert call(a) == _native.E_ALIAS, (name, other, shift)
        assert name in _native.last_error() and other in _native.last_error()
    # the first byte past an array is not an overlap
    a = _fake_args(C, D, md)
    a.q_out = a.prop + C * D * 8
    a.C = 0                                                    # ... and C == 0 is no error, and no launch
    assert call(a) == 0


def test_pending_and_adapt_step_refusals():
    L = _native.lib()
    fake = [(i + 1) << 40 for i in range(6)]
    assert L.binf_nuts_pending(fake[0], -1, fake[1], None) == _native.E_ARG
    assert L.binf_nuts_pending(fake[0], 4, None, None) == _native.E_ARG
    assert L.binf_nuts_pending(None, 4, fake[1], None) == _native.E_ARG
    ok = lambda action, C=4, acc=fake[1]: L.binf_nuts_adapt_step_f64(fake[0], acc, fake[2], fake[3], fake[4], fake[5],
                                                                     0.8, 0.1, 1.0, 1.0, action, C, None)
    assert ok(3) == _native.E_ARG and ok(-1) == _native.E_ARG
    assert ok(0, C=-1) == _native.E_ARG
    assert ok(0, acc=None) == _native.E_ARG
    assert ok(0, C=0) == 0


def test_sampler_refuses_what_it_does_not_do():
    from binf_amd.samplers import NUTSSampler
    from binf_amd.samplers.hmc import HMCSampler
    assert issubclass(NUTSSampler, HMCSampler)
    with pytest.raises(ValueError, match='graph'):
        NUTSSampler(None, None, 0.1, graph=True)
    with pytest.raises(ValueError, match='nsteps'):
        NUTSSampler(None, None, 0.1, nsteps=5)
    with pytest.raises(ValueError, match='max_tree_depth'):
        NUTSSampler(None, None, 0.1, max_tree_depth=13)

    class Mine(NUTSSampler):
        def _leapfrog(self, q, p, timestep, nsteps):
            return q, p
    with pytest.raises(TypeError, match='_leapfrog'):
        Mine(None, None, 0.1)
    s = NUTSSampler(None, None, 0.1, max_tree_depth=4, variable_name='x')
    assert s.max_tree_depth == 4 and s.graph is False and s.variable_name == 'x'
