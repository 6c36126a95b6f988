"""Tempered SMC on the device (``csrc/smc.hip``, ``binf_amd/samplers/smc.py``) against the host
restatement ``tests/smc_ref.py``: the gather bit for bit, the resampler as integers and by the
properties no biased resampler has, the temper kernel's discrete choice against 100-digit
arithmetic and its floating outputs inside derived bounds, one stage of the class against
the three kernels composed, checkpoint / resume, and the evidence of a conjugate Gaussian."""
import numpy as np
import pytest
import torch

import smc_ref as R
from binf_amd import _native, checkpoint
from binf_amd.samplers.hmc import HMCSampler
from binf_amd.samplers.rng import DeviceRNG
from binf_amd.samplers.smc import SMCResult, TemperedSMC

pytestmark = pytest.mark.gpu

SENT = -7.25                       # sentinel of the double buffers
SENT_I = -99
f64 = np.float64


def dev(a, device):
    return torch.from_numpy(np.ascontiguousarray(a)).to(device)


def ptr(t):
    return None if t is None else t.data_ptr()


def carve(a, device, before=0, after=0, fill=None):
    """``a`` on the device inside a larger sentinel-filled buffer: (view, whole buffer).
    ``before`` elements in front shift a double view off 16-byte alignment when odd."""
    flat = np.ascontiguousarray(a).reshape(-1)
    if fill is None:
        fill = SENT if flat.dtype == np.float64 else SENT_I
    whole = torch.full((before + flat.size + after,), fill, dtype=torch.from_numpy(flat[:0]).dtype,
                       device=device)
    view = whole[before:before + flat.size]
    view.copy_(torch.from_numpy(flat))
    return view, whole


def guards_intact(whole, before, n):
    w = whole.cpu().numpy()
    fill = SENT if w.dtype == np.float64 else SENT_I
    return bool(np.all(w[:before] == fill) and np.all(w[before + n:] == fill))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.all(a.view(np.int64) == b.view(np.int64)))


# ---------------------------------------------------------------------------
# the gather
# ---------------------------------------------------------------------------
@pytest.mark.parametrize('D', [1, 3, 4, 1023, 1024])
@pytest.mark.parametrize('C', [1, 5, 256])
def test_gather_is_x_of_ancestor_bit_for_bit(device, C, D):
    L = _native.lib()
    rs = np.random.RandomState(1000 * C + D)
    x = rs.standard_normal((C, D))
    x.reshape(-1)[::7] = -0.0
    x.reshape(-1)[3::11] = np.nan
    side = rs.standard_normal((4, C))
    for case, (sx, so, K) in enumerate([(0, 0, 0), (1, 0, 1), (0, 1, 4), (1, 1, 4), (2, 3, 2)]):
        anc = rs.randint(0, C, size=C).astype(np.int64)
        if case == 0:
            anc = np.arange(C, dtype=np.int64)
        xd, xw = carve(x, device, before=sx, after=3)
        od, ow = carve(np.full((C, D), SENT), device, before=so, after=5)
        sd, _ = carve(side[:K], device, before=1, after=1)
        sod, sow = carve(np.full((K, C), SENT), device, before=3, after=3)
        ad, aw = carve(anc, device, before=1, after=1)
        x_before = xw.clone()
        rc = L.binf_smc_gather_f64(ptr(xd), ptr(ad), ptr(od), ptr(sd) if K else None, ptr(sod) if K else None,
                                   K, C, D, _native.stream_handle(device))
        assert rc == 0, _native.last_error()
        torch.cuda.synchronize()
        assert same_bits(od.cpu().numpy().reshape(C, D), x[anc]), (sx, so, K)
        if K:
            assert same_bits(sod.cpu().numpy().reshape(K, C), side[:K][:, anc])
        assert guards_intact(ow, so, C * D) and guards_intact(sow, 3, K * C) and guards_intact(aw, 1, C)
        assert torch.equal(xw.view(torch.int64), x_before.view(torch.int64))       # x is never written


def test_gather_refusals_and_foreign_ancestors(device):
    L = _native.lib()
    C, D = 6, 5
    x = dev(np.arange(C * D, dtype=f64).reshape(C, D), device)
    anc = dev(np.array([0, 5, -1, 6, 2, 2], dtype=np.int64), device)
    s = _native.stream_handle(device)
    buf = torch.full((2 * C * D,), SENT, dtype=torch.float64, device=device)
    assert L.binf_smc_gather_f64(ptr(buf), ptr(anc), ptr(buf[C * D - 1:]), None, None, 0, C, D, s) == _native.E_ALIAS
    assert L.binf_smc_gather_f64(ptr(x), ptr(anc), ptr(x), None, None, 0, C, D, s) == _native.E_ALIAS
    with pytest.raises(ValueError):
        _native.smc_gather(x, anc, out=x)
    torch.cuda.synchronize()
    assert bool((buf == SENT).all())                          # a refusal touches nothing
    # an ancestor outside [0, C): the row is quiet NaN, every other row is served
    side = dev(np.arange(C, dtype=f64)[None, :] + 0.5, device)
    out, so = _native.smc_gather(x, anc, side=side)
    o, xs = out.cpu().numpy(), x.cpu().numpy()
    for c, a in enumerate([0, 5, -1, 6, 2, 2]):
        if 0 <= a < C:
            assert np.array_equal(o[c], xs[a]) and float(so[0, c]) == a + 0.5
        else:
            assert np.all(np.isnan(o[c])) and np.isnan(float(so[0, c]))


# ---------------------------------------------------------------------------
# the resampler
# ---------------------------------------------------------------------------
def run_resample(device, w, P, u=None, status=None, seed=0, offset=0, chain_offset=0):
    """One call through the C ABI with guarded outputs: numpy (ancestor [C], n_unique [G])."""
    L = _native.lib()
    C = w.shape[0]
    G = C // P
    wd = dev(w, device)
    ad, aw = carve(np.full(C, SENT_I, dtype=np.int64), device, before=1, after=2)
    nd, nw = carve(np.full(G, SENT_I, dtype=np.int64), device, before=1, after=2)
    ud = None if u is None else dev(np.asarray(u, dtype=f64), device)
    sd = None if status is None else dev(np.asarray(status, dtype=np.int32), device)
    rc = L.binf_smc_resample_f64(ptr(wd), ptr(ud), ptr(sd), C, P, G, seed, offset, chain_offset,
                                 ptr(ad), ptr(nd), _native.stream_handle(device))
    assert rc == 0, _native.last_error()
    torch.cuda.synchronize()
    assert guards_intact(aw, 1, C) and guards_intact(nw, 1, G)
    return ad.cpu().numpy(), nd.cpu().numpy()


@pytest.mark.parametrize('P', [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4096])
@pytest.mark.parametrize('G', [1, 3])
def test_resampler_equals_the_restatement_and_has_its_properties(device, P, G):
    n_pat = len(R.PATTERNS)
    for k in range(n_pat):
        kinds = [R.PATTERNS[(k + g) % n_pat] for g in range(G)]
        w = np.concatenate([R.weight_pattern(P, kind, 100 * P + 7 * g + k) for g, kind in enumerate(kinds)])
        for j, u0 in enumerate(R.U_EDGE):
            u = np.array([R.U_EDGE[(j + g) % 3] for g in range(G)])
            anc, n_unique = run_resample(device, w, P, u=u)
            want_anc, want_unique = R.resample_batch(w, u, P)
            assert np.array_equal(anc, want_anc), (kinds, u)
            assert np.array_equal(n_unique, want_unique), (kinds, u)
            # on the device output itself
            for g in range(G):
                a = anc[g * P:(g + 1) * P] - g * P
                wg = w[g * P:(g + 1) * P]
                assert a.min() >= 0 and a.max() < P and np.all(np.diff(a) >= 0)
                assert np.all(wg[a] > 0.0), 'a particle of weight 0 became an ancestor'
                assert R.count_rule_holds(wg, a), (kinds[g], u[g])
                assert n_unique[g] == len(set(a.tolist()))


@pytest.mark.parametrize('P', [63, 257, 1000])
def test_resampler_mean_counts_over_256_draws(device, P):
    """256 populations of the same weights, one independent uniform each: the number of draws
    in which particle i got ceil(P w_i / total) copies is Binomial(256, frac(P w_i / total)) and
    must lie in that law's central interval (1e-9 in each tail, exact pmf).  A resampler whose
    targets sit off by a fraction of a slot fails it (tests/test_smc.py shows one failing)."""
    w = R.weight_pattern(P, 'zero_runs', 5 * P)
    us = np.random.RandomState(P).uniform(size=256)
    anc, _ = run_resample(device, np.tile(w, 256), P, u=us)
    rows = anc.reshape(256, P) - (np.arange(256) * P)[:, None]
    assert R.mean_count_rule_holds(w, rows)


def test_resampler_draws_in_the_kernel_by_global_chain_index(device):
    P, G = 257, 4
    w = np.concatenate([R.weight_pattern(P, 'random', 40 + g) for g in range(G)])
    seed, offset = 1234, 9
    whole, nu = run_resample(device, w, P, seed=seed, offset=offset)
    part, nu_part = run_resample(device, w[2 * P:], P, seed=seed, offset=offset, chain_offset=2 * P)
    assert np.array_equal(part + 2 * P, whole[2 * P:]) and np.array_equal(nu_part, nu[2:])
    # the draw is element g * P of the uniform stream (seed, offset)
    stream = torch.empty(G * P, dtype=torch.float64, device=device)
    _native.rng_fill('uniform', stream, seed, offset)
    u = stream.cpu().numpy()[::P]
    assert np.all((u >= 0.0) & (u < 1.0)) and len(set(u.tolist())) == G
    fed, _ = run_resample(device, w, P, u=u)
    assert np.array_equal(fed, whole)
    other, _ = run_resample(device, w, P, seed=seed, offset=offset + 1)
    assert not np.array_equal(other, whole)


def test_resampler_identity_paths(device):
    P = 65
    w = np.concatenate([R.weight_pattern(P, 'random', g) for g in range(6)])
    w[4 * P:5 * P] = 0.0                                      # no positive total
    w[5 * P] = np.inf                                         # no finite total
    status = [R.OK, R.FINISHED, R.NO_FINITE, R.INVALID, R.OK, R.STALLED]
    anc, nu = run_resample(device, w, P, u=[0.25] * 6, status=status)
    ident = np.arange(6 * P)
    for g in (1, 2, 3, 4, 5):
        assert np.array_equal(anc[g * P:(g + 1) * P], ident[g * P:(g + 1) * P]) and nu[g] == P
    assert not np.array_equal(anc[:P], ident[:P])
    for bad in (1.0, -0.25, np.nan, np.inf):                 # a supplied u outside [0, 1)
        anc, nu = run_resample(device, w[:P], P, u=[bad])
        assert np.array_equal(anc, ident[:P]) and nu[0] == P


# ---------------------------------------------------------------------------
# the temper kernel
# ---------------------------------------------------------------------------
def run_temper(device, ll, beta, P, rho=0.5, n_bisect=60):
    """One call through the C ABI with guarded outputs: dict of numpy arrays."""
    L = _native.lib()
    C = ll.shape[0]
    G = C // P
    lld = dev(ll, device)
    bd, bw = carve(np.asarray(beta, dtype=f64), device, before=1, after=1)
    outs = {}
    for name, n, dt in (('delta', G, f64), ('beta_chain', C, f64), ('w', C, f64), ('log_z_inc', G, f64),
                        ('ess', G, f64), ('n_invalid', G, np.int64), ('status', G, np.int32)):
        outs[name] = carve(np.full(n, SENT if dt is f64 else SENT_I, dtype=dt), device, before=1, after=3) + (n,)
    o = {k: v[0] for k, v in outs.items()}
    rc = L.binf_smc_temper_f64(ptr(lld), ptr(bd), C, P, G, rho, n_bisect, ptr(o['delta']), ptr(o['beta_chain']),
                               ptr(o['w']), ptr(o['log_z_inc']), ptr(o['ess']), ptr(o['n_invalid']),
                               ptr(o['status']), _native.stream_handle(device))
    assert rc == 0, _native.last_error()
    torch.cuda.synchronize()
    assert guards_intact(bw, 1, G)
    for name, (view, whole, n) in outs.items():
        assert guards_intact(whole, 1, n), name
    res = {k: v.cpu().numpy() for k, v in o.items()}
    res['beta'] = bd.cpu().numpy()
    return res


def check_against_restatement_at_device_delta(ll, got, g, P):
    """(b): w, ess and log_z_inc of population ``g`` against the restatement evaluated AT THE
    DEVICE'S delta.  Both sides form e = l - m and d * e with the same roundings, so a weight
    differs by the two exps alone: each within an ulp of the exact value t, an ulp of t being at
    most 2^-52 t and t <= w_ref / (1 - 2^-52) (2 quanta where t is subnormal); the sums follow
    smc_ref.sum_bounds / ess_bound / log_z_bound with sides=2."""
    sl = slice(g * P, (g + 1) * P)
    d = got['delta'][g]
    want = R.temper_at(ll[sl], d)
    w = got['w'][sl]
    assert np.all(np.abs(w - want['w']) <= 2.0 * R.EPS * (1.0 + 2.0 * R.EPS) * want['w'] + 2.0 * 2.0 ** -1074)
    dead = ~np.isfinite(ll[sl])
    assert np.all(w[dead] == 0.0) and not np.any(np.signbit(w[dead])), 'weight of -inf / NaN is not +0.0'
    s1, s2 = want['s1'], want['s2']
    assert abs(got['ess'][g] - want['ess']) <= R.ess_bound(P, s1, s2)
    assert abs(got['log_z_inc'][g] - want['log_z_inc']) <= R.log_z_bound(P, s1, s2, want['log_z_inc'])
    return want


def check_bracket(ll, got, g, P, beta, rho, n_bisect):
    """(a): with 100-digit arithmetic, ESS(delta) >= rho P - eps and ESS(delta + hi0 2^-n) <=
    rho P + eps.  The device accepted ``enough(delta)`` and refused ``enough(hi)`` in floating
    point, hi - delta = hi0 2^-n up to 2^-52 hi0 (each midpoint rounds by half an ulp of a value <=
    hi0, and the errors halve with the bracket).  eps = the error of a device ESS against exact
    arithmetic, smc_ref.ess_bound(sides=1): an ulp of exp and the roundings of l - m and d * e per
    weight (under 2 * 2^-52 absolute), 5 * 2^-52 per squared weight, half an ulp of the partial
    sum per addition along THE SUM's sum_depth(P) levels, the two roundings of S1 * S1 / S2; +
    2^-53 rho P for the rounding of rho * P; + |dESS / d delta| <= 2 P max|e| (smc_ref.slope_bound)
    times the 2^-52 hi0 by which hi may differ from delta + hi0 2^-n."""
    import mpmath
    sl = slice(g * P, (g + 1) * P)
    d = float(got['delta'][g])
    hi0 = 1.0 - beta
    m, e = R.shifted(ll[sl])
    _, s1, s2, _ = R.sums(e, d)
    eps = R.ess_bound(P, s1, s2, sides=1) + R.slope_bound(P, e) * R.EPS * hi0 + 0.5 * R.EPS * rho * P
    assert eps < 1e-6 * P
    assert R.exact_ess(ll[sl], mpmath.mpf(d)) >= rho * P - eps
    step = mpmath.mpf(hi0) * mpmath.mpf(2) ** -n_bisect
    assert R.exact_ess(ll[sl], mpmath.mpf(d) + step) <= rho * P + eps


@pytest.mark.parametrize('P', [1, 2, 64, 257, 4096, 8200])
def test_temper_step_brackets_the_root_and_outputs_meet_their_bounds(device, P):
    """Three populations in one call -- a plain one at beta 0, one with -inf / NaN holes at beta
    0.25, a plain one at 0.5 with 20 halvings asked of all -- and the first alone: (a) the
    discrete choice against exact arithmetic, (b) the floating outputs at the device's delta,
    and the same bits whatever G.  P = 8200 is past the kernel's LDS threshold."""
    rho = 0.5
    lls = [R.ll_sample(P, 'plain', 11 * P), R.ll_sample(P, 'holes', 3 * P), R.ll_sample(P, 'plain', 5 * P + 1)]
    betas = [0.0, 0.25, 0.5]
    ll = np.concatenate(lls)
    for n_bisect in (60, 20):
        got = run_temper(device, ll, betas, P, rho, n_bisect)
        for g in range(3):
            want = check_against_restatement_at_device_delta(ll, got, g, P)
            d = got['delta'][g]
            assert got['n_invalid'][g] == int(np.isnan(lls[g]).sum())
            assert np.all(got['beta_chain'][g * P:(g + 1) * P] == got['beta'][g])
            assert got['status'][g] == R.OK
            if want['ess'] >= rho * P and d == 1.0 - betas[g]:
                assert got['beta'][g] == 1.0                  # the last step fits: exactly 1
            else:
                assert 0.0 < d < 1.0 - betas[g] and got['beta'][g] == betas[g] + d
                if P <= 4096 or g == 0:
                    check_bracket(ll, got, g, P, betas[g], rho, n_bisect)
        if P <= 2:
            assert np.all(got['beta'] == 1.0)                 # ESS >= 1 >= rho P at any step
        else:
            assert np.all(got['beta'] < 1.0)                  # these likelihoods need several stages
        alone = run_temper(device, lls[0], betas[:1], P, rho, n_bisect)
        for name in ('delta', 'beta', 'log_z_inc', 'ess'):
            assert same_bits(alone[name], got[name][:1]), name
        assert same_bits(alone['w'], got['w'][:P]) and same_bits(alone['beta_chain'], got['beta_chain'][:P])


def test_temper_lands_on_one_and_every_status_path(device):
    P = 64
    rs = np.random.RandomState(5)
    flat = -0.05 * rs.uniform(size=P)                         # nearly equal weights: any step fits
    stalled = np.full(P, -1e30)
    stalled[0] = 0.0
    pinf = flat.copy()
    pinf[3], pinf[9] = np.inf, np.nan
    none = np.full(P, -np.inf)
    none[::4] = np.nan
    done = rs.standard_normal(P) * 50.0
    ll = np.concatenate([flat, flat, stalled, pinf, none, done])
    betas = [0.0, 0.8125, 0.0, 0.5, 0.25, 1.0]
    got = run_temper(device, ll, betas, P, 0.5, 60)
    assert got['status'].tolist() == [R.OK, R.OK, R.STALLED, R.INVALID, R.NO_FINITE, R.FINISHED]
    assert got['beta'].tolist() == [1.0, 1.0, 2.0 ** -60, 0.5, 0.25, 1.0]
    assert got['delta'].tolist() == [1.0, 0.1875, 2.0 ** -60, 0.0, 0.0, 0.0]
    assert got['n_invalid'].tolist() == [0, 0, 0, 1, P // 4, 0]
    for g in (3, 4, 5):                                       # pass-through
        assert np.all(got['w'][g * P:(g + 1) * P] == 1.0)
        assert got['log_z_inc'][g] == 0.0 and got['ess'][g] == P
    for g in range(6):
        assert np.all(got['beta_chain'][g * P:(g + 1) * P] == got['beta'][g])
        want = R.temper(ll[g * P:(g + 1) * P], betas[g], 0.5, 60)
        assert want['status'] == got['status'][g] and want['delta'] == got['delta'][g]
        assert want['beta'] == got['beta'][g] and want['n_invalid'] == got['n_invalid'][g]
    # the stalled population: one particle carries everything, ESS = 1
    assert got['ess'][2] == 1.0
    assert abs(got['log_z_inc'][2] + np.log(f64(P))) <= 2.0 * R.EPS * np.log(f64(P))      # an ulp of log per side
    assert np.all(got['w'][2 * P + 1:3 * P] == 0.0)
    for g in (0, 1):
        check_against_restatement_at_device_delta(ll, got, g, P)


# ---------------------------------------------------------------------------
# the class
# ---------------------------------------------------------------------------
S0, S, Y = R.E2E['prior_sd'], R.E2E['noise_sd'], R.E2E['y']


class TemperedGaussian(object):
    """log p_beta(x) = log N(x | 0, S0^2 I) + beta_c log N(Y 1 | x, S^2 I); ``beta`` is the [C]
    device tensor the SMC writes."""
    variables = {'x'}

    def __init__(self, beta, D):
        self.beta, self.D = beta, D

    def log_likelihood(self, x):
        return -0.5 * ((x - Y) ** 2).sum(dim=1) / S ** 2 - 0.5 * self.D * float(np.log(2.0 * np.pi * S ** 2))

    def log_prob(self, x):
        prior = -0.5 * (x * x).sum(dim=1) / S0 ** 2 - 0.5 * self.D * float(np.log(2.0 * np.pi * S0 ** 2))
        return prior + self.beta * self.log_likelihood(x)

    def gradient(self, x):
        return x / S0 ** 2 + self.beta[:, None] * (x - Y) / S ** 2


def set_dt(smc):
    smc.sampler.timestep = 0.5 / torch.sqrt(1.0 / S0 ** 2 + smc.beta / S ** 2)


def build(device, G, P, seed, D=R.E2E['D'], explicit=False, n_mutations=R.E2E['n_mutations'], **kw):
    C = G * P
    rng = DeviceRNG(seed, device)
    beta = torch.zeros(C, dtype=torch.float64, device=device)
    pdf = TemperedGaussian(beta, D)
    start = rng.normal((C, D), device) * S0
    inner = HMCSampler(pdf, start, 0.1, R.E2E['n_steps'], variable_name='x', rng=rng)
    smc = TemperedSMC(inner, beta, n_populations=G, ess_fraction=R.E2E['rho'], n_mutations=n_mutations,
                      log_likelihood=pdf.log_likelihood if explicit else None, before_mutation=set_dt, **kw)
    return smc, pdf, inner, rng


def test_one_stage_is_the_three_kernels_composed(device):
    """Two stages through the class (the generic log-likelihood: log_prob at beta 1 minus
    log_prob at beta 0) against temper -> resample -> gather -> two transitions written here,
    bit for bit, u supplied."""
    G, P = 3, 257
    smc, pdf, inner, rng = build(device, G, P, seed=3)
    _, pdf2, inner2, rng2 = build(device, G, P, seed=3)
    beta_pop = torch.zeros(G, dtype=torch.float64, device=device)
    log_z = torch.zeros(G, dtype=torch.float64, device=device)
    for stage in range(2):
        u = dev(np.array([0.125, 0.5, 0.875]) / (stage + 1), device)
        x0 = smc.state
        out = smc.step(u=u)
        # composed
        x = inner2.state
        assert torch.equal(x, x0)
        pdf2.beta.fill_(1.0)
        lp1 = pdf2.log_prob(x)
        pdf2.beta.fill_(0.0)
        ll = (lp1 - pdf2.log_prob(x)).contiguous()
        t = _native.smc_temper(ll, beta_pop, pdf2.beta, R.E2E['rho'], 60)
        anc, n_unique = _native.smc_resample(t['w'], G, u=u, status=t['status'])
        moved, side = _native.smc_gather(x, anc, side=ll.view(1, -1))
        inner2.state = moved
        inner2.timestep = 0.5 / torch.sqrt(1.0 / S0 ** 2 + pdf2.beta / S ** 2)
        inner2.sample_n(2, record=False)
        log_z = log_z + t['log_z_inc']
        assert torch.equal(out.view(torch.int64), inner2.state.view(torch.int64))
        assert torch.equal(smc.beta, pdf2.beta) and torch.equal(smc.beta_population, beta_pop)
        assert torch.equal(smc.log_evidence.view(torch.int64), log_z.view(torch.int64))
        assert torch.equal(smc.last['ancestor'], anc) and torch.equal(smc.last['n_unique'], n_unique)
        assert torch.equal(smc.last['log_likelihood'], ll[anc])
        assert not torch.equal(anc, torch.arange(G * P, device=device))
        assert x0.data_ptr() != out.data_ptr() and torch.equal(x0, x)       # the old state is not written
    r = smc.result()
    assert isinstance(r, SMCResult) and r.betas.shape == (2, G) and r.n_unique.dtype == torch.int64
    assert torch.equal(r.n_stages, torch.full((G,), 2, dtype=torch.int64, device=device))
    assert 'log_evidence' in str(r)
    assert rng.offset == rng2.offset


def test_checkpoint_between_stages_resumes_bit_for_bit(device):
    G, P = 2, 256
    a, _, _, _ = build(device, G, P, seed=11, explicit=True)
    a.step()
    a.step()
    ckpt = checkpoint.state_dict(smc=a)
    for _ in range(2):
        a.step()
    b, pdf_b, _, _ = build(device, G, P, seed=999, explicit=True)
    checkpoint.load_state_dict(ckpt, smc=b)
    assert torch.equal(pdf_b.beta.view(G, P)[:, 0], b.beta_population) and b.stage == 2
    for _ in range(2):
        b.step()
    ra, rb = a.result(), b.result()
    assert torch.equal(a.state.view(torch.int64), b.state.view(torch.int64))
    for name in ('log_evidence', 'betas', 'ess'):
        assert torch.equal(getattr(ra, name).view(torch.int64), getattr(rb, name).view(torch.int64)), name
    assert torch.equal(ra.n_unique, rb.n_unique) and torch.equal(ra.n_stages, rb.n_stages)
    assert ra.betas.shape == (4, G)


def test_class_refusals(device):
    smc, pdf, inner, rng = build(device, 2, 8, seed=1)
    with pytest.raises(ValueError):
        TemperedSMC(inner, pdf.beta, n_populations=3)
    with pytest.raises(ValueError):
        TemperedSMC(inner, pdf.beta, n_populations=2, ess_fraction=0.0)
    uneven = pdf.beta.clone()
    uneven[3] = 0.5
    with pytest.raises(ValueError):
        TemperedSMC(inner, uneven, n_populations=2)
    with pytest.raises(ValueError):
        TemperedSMC(inner, pdf.beta, n_populations=2, rng=DeviceRNG(0, device, chain_offset=4))
    inner.pools_chains_to_adapt, inner.adapting = True, True
    with pytest.raises(TypeError):
        TemperedSMC(inner, pdf.beta, n_populations=2)
    TemperedSMC(inner, pdf.beta, n_populations=1)             # one population may pool
    inner.adapting = False
    TemperedSMC(inner, pdf.beta, n_populations=2)
    stuck = TemperedSMC(inner, pdf.beta, n_populations=2, max_stages=1, n_mutations=0,
                        log_likelihood=lambda x: -1e3 * (x * x).sum(dim=1))
    with pytest.raises(RuntimeError):
        stuck.run()


def test_evidence_of_the_conjugate_gaussian(device):
    """Prior N(0, 3^2 I_4), likelihood N(y = 2 1 | x, 0.5^2 I_4), G = 16 populations of P = 256,
    rho = 0.5, two HMC transitions of 8 steps per stage at dt = 0.5 / sqrt(1/9 + 4 beta);
    analytic log Z = -8.98987.

    Yardstick: tests/smc_ref.py's whole-loop restatement on the CPU, 200 seeds (tests/
    test_smc.py re-runs it): mean -9.0037, sd s = 0.16297 per population, at most 6 stages.
    Asserted: |mean over the 16 populations - analytic| <= 5 s / sqrt(16) + s^2 / 2 = 0.2170
    (the second term is the known bias of log Z), every population done in <= 12 stages, betas
    strictly increasing and ending in 1.0.

    Control: the same mutation with the reweighting skipped -- no resampling, log_z_inc forced
    to delta * mean(l), the thermodynamic-integration integrand at the stage's start.  On the CPU
    the control gives -14.690 +- 0.243 per population, 5.70 below the analytic value, 26 times
    the bound; it must miss the bound here too."""
    G, P = R.E2E['G'], R.E2E['P']
    bound = R.e2e_bound()
    assert abs(bound - 0.2170) < 1e-4
    smc, pdf, inner, rng = build(device, G, P, seed=2024, explicit=True, max_stages=50)
    r = smc.run().cpu()
    lz = r.log_evidence.numpy()
    print('log_evidence per population', lz, 'mean', lz.mean(), 'stages', r.n_stages.numpy())
    assert abs(lz.mean() - R.e2e_analytic()) <= bound
    assert int(r.n_stages.max()) <= 12 and r.betas.shape[0] <= 12
    b = np.concatenate([np.zeros((1, G)), r.betas.numpy()])
    for g in range(G):
        n = int(r.n_stages[g])
        assert np.all(np.diff(b[:n + 1, g]) > 0.0) and b[n, g] == 1.0 and np.all(b[n:, g] == 1.0)
    assert set(r.status.numpy().tolist()) <= {R.OK, R.FINISHED}
    assert abs(float(r.log_evidence_mean) - np.log(np.mean(np.exp(lz)))) < 1e-12
    assert abs(float(r.stderr) - lz.std(ddof=1) / 4.0) < 1e-12
    assert float(r.ess.min()) >= 0.5 * P - 1e-6 and int(r.n_unique.min()) > P // 8
    # the posterior itself: N(y s0^2 / (s0^2 + s^2), s0^2 s^2 / (s0^2 + s^2)) per coordinate
    x = smc.state.cpu().numpy()
    v = S0 ** 2 * S ** 2 / (S0 ** 2 + S ** 2)
    assert abs(x.mean() - Y * S0 ** 2 / (S0 ** 2 + S ** 2)) < 6.0 * np.sqrt(v / (G * P * 4) * 8.0)

    # control
    ctl, pdf_c, inner_c, _ = build(device, G, P, seed=2024, explicit=True)
    beta_pop = torch.zeros(G, dtype=torch.float64, device=device)
    log_z = torch.zeros(G, dtype=torch.float64, device=device)
    for stage in range(50):
        ll = pdf_c.log_likelihood(inner_c.state).contiguous()
        t = _native.smc_temper(ll, beta_pop, pdf_c.beta, R.E2E['rho'], 60)
        log_z = log_z + t['delta'] * ll.view(G, P).mean(dim=1)
        set_dt(ctl)
        inner_c.sample_n(R.E2E['n_mutations'], record=False)
        if bool((beta_pop >= 1.0).all()):
            break
    miss = abs(float(log_z.mean()) - R.e2e_analytic())
    print('control mean', float(log_z.mean()), 'miss', miss)
    assert bool((beta_pop >= 1.0).all()) and miss > bound


def test_example_runs(device):
    """examples/smc_evidence.py at its default size: both estimates within five of their own
    standard errors plus the bias sd^2 / 2 = G stderr^2 / 2 of log Z."""
    import importlib.util
    import os
    from conftest import ROOT
    spec = importlib.util.spec_from_file_location('example_smc_evidence',
                                                  os.path.join(ROOT, 'examples', 'smc_evidence.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(populations=16, particles=256, quiet=True)
    assert set(out) == {'gaussian', 'double_well'}
    for name, (r, exact) in out.items():
        h = r.cpu()
        lz = h.log_evidence.numpy()
        se = float(h.stderr)
        print(name, 'mean', lz.mean(), 'stderr', se, 'exact', exact, 'stages', h.n_stages.numpy())
        assert abs(lz.mean() - exact) <= 5.0 * se + 0.5 * 16 * se * se, name
        assert bool((h.betas[-1] == 1.0).all()) and int(h.n_stages.max()) <= 40, name
