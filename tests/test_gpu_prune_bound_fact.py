"""The fp32 bound kernel's sign-homogeneous row tiles and factorised exponent on the device (k_bound_mfma32<KS, NC, FACT>, k_bound_aug's
row order, k_bound_guard's range guard; csrc/bound_f32.h).  The host side of the same proof is
tests/test_bound_f32_fact_host.py.

Held here, under prune_bound = -1 at M = 131072 (the smallest sweep that takes the fp32 kernel by its guards) unless said otherwise:

  margin and form   d in {1, 3, 5, 8, 9, 12, 16, 18} -- every <KS, NC> instance -- at N = Np (no padding row: only the extra zero tile
                    separates the signs, and Np / 16 + 1 tiles is odd, so the waves' tile counts differ) and N = Np - 1: against the fp64
                    matrix-pipe kernel's dots (prune_bound = 1) of the same engine, every candidate,
                        dots32 >= dots64 - eps_k rho S          dots32 - dots64 <= 2 E B_n + eps_k rho S + 3 F
                    (B_n = sum |w_i| k_i in fp64 from the device's T and a, taken 1e-9 larger; F the flush term of bound_f32.h from the
                    report's S); the report says bound_fact; the pruned top-k is array_equal to the plain one for k in {1, 10, 64};
                    tpos = ceil(npos / 16) from the weights read back;
  sign patterns     all weights positive, all negative (y - bias of one sign under a dominant noise term), all zero (y = bias): margin
                    and top-k again, tpos = ceil(N / 16), 0 and 0;
  fallback          a model whose weights are normal in fp32 while some w' = w r_i is not (under -1), and a model and candidate set with
                    L R_x R_z > 120 while E <= 2^-10 (forced, prune_bound = 2, M = 3 G + 77): bound_fact is false, the margin holds and the
                    dots are those of the same handle with option bound_fact = 0, bit for bit;
  edges             a candidate on an observation, one with a NaN coordinate, one 100 length scales away keep what
                    tests/test_gpu_prune_bound_f32.py asserts of them, with bound_fact = 1 and 0;
  ensemble          three members of different hyperparameters, the fp32 kernel on each: pruned equals plain, every member reports its form."""
import numpy as np
import pytest

from test_gpu_prune import _dev
from test_gpu_prune_bound import _engine, _problem, check_sweep
from test_gpu_prune_bound_mfma import _eps_k

pytestmark = pytest.mark.gpu

G = 4096
E_MAX = 2.0 ** -10
M32 = 131072
W_MIN = 2.0 ** -126
LOG2E = 1.4426950408889634


def _signed_weights(e, w):
    """w_i = rho alpha~_i, alpha~ = T^T a from the device's factor inverse and a."""
    T, a = e.get_matrix('T'), e.get_vectors()[0]
    return w['rho'] * (T.T @ a)


def _B(w, absw, Z):
    """B_n = sum_i |w_i| k(x_i, z_n) in fp64 on the device (torch), taken 1e-9 larger: the expansion's and the sum's own rounding."""
    import torch
    inv = 1.0 / w['ell']
    Xs = torch.as_tensor(w['X'] * inv, device='cuda')
    Zs = torch.as_tensor(np.nan_to_num(Z * inv, nan=0.0, posinf=1e150, neginf=-1e150), device='cuda')
    aw = torch.as_tensor(absw, device='cuda')
    x2 = (Xs ** 2).sum(1)
    out = torch.empty(len(Z), dtype=torch.float64, device='cuda')
    for j0 in range(0, len(Z), 16384):
        z = Zs[j0:j0 + 16384]
        r2 = torch.clamp(x2[:, None] + (z ** 2).sum(1)[None, :] - 2.0 * (Xs @ z.T), min=0.0)
        out[j0:j0 + 16384] = aw @ torch.exp(-0.5 * r2)
    return out.cpu().numpy() * (1.0 + 1e-9)


def _dots(e, Z, k, bound, fact=1):
    e.set_option('prune', 1)
    e.set_option('prune_bound', bound)
    e.set_option('bound_fact', fact)
    dZ = _dev(Z)
    e.sweep_dev('ei', e.mean_at_obs()[1], dZ.data_ptr(), len(Z), k)
    r = e.prune_report(vectors=False)
    dots = e.prune_dots()
    e.set_option('bound_fact', 1)
    return r, dots


def _flush(r, Np, rho):
    return 2.0 ** -124 * (rho * r['S'] * (1.0 + 2.0 ** -20) + Np)


def _margin(e, w, Z, r32, d32, label):
    """dots32 against the fp64 matrix-pipe kernel's dots, every candidate."""
    r64, d64 = _dots(e, Z, 10, 1)
    assert r64['bound_kernel'] == 'mfma' and np.isnan(r64['E']) and r64['bound_fact'] is None, label
    assert np.array_equal(np.isnan(d32), np.isnan(d64)), label
    ok = ~np.isnan(d64)
    E = r32['E']
    assert 0.0 < E <= E_MAX, (label, E)
    Np = (w['N'] + 127) // 128 * 128
    room = _eps_k(w['d'], r64['guard']) * w['rho'] * r64['S']
    F = _flush(r32, Np, w['rho'])
    sw = _signed_weights(e, w)
    B = _B(w, np.abs(sw), Z)
    low = d32[ok] - d64[ok]
    print('%-34s fact %-5s tpos %3s E %.3e  min (d32 - d64) %.3e  max (d32 - d64) / (2 E B + 3 F) %.4f  eps_k rho S %.3e' %
          (label, r32['bound_fact'], r32['bound_tpos'], E, float(low.min()), float(np.max(low / (2.0 * E * B[ok] + 3.0 * F))), room))
    assert np.all(low >= -room), (label, float(low.min()), room)
    assert np.all(low <= 2.0 * E * B[ok] + room + 3.0 * F), (label, float(np.max(low - 2.0 * E * B[ok])), room, F)
    return sw


def _topk_equal(e, Z, ks, label):
    dZ = _dev(Z)
    target = e.mean_at_obs()[1]
    for k in ks:
        e.set_option('prune', 0)
        plain = e.sweep_dev('ei', target, dZ.data_ptr(), len(Z), k)
        e.set_option('prune', 1)
        got = e.sweep_dev('ei', target, dZ.data_ptr(), len(Z), k)
        assert e.prune_report(vectors=False)['bound_kernel'] == 'mfma32', (label, k)
        assert np.array_equal(got[0], plain[0], equal_nan=True) and np.array_equal(got[1], plain[1]), (label, k)


def _tpos_of(sw):
    return (int(np.sum(sw > 0.0)) + 15) // 16


CASES = [(d, N) for d, Np in ((1, 384), (3, 384), (5, 384), (8, 1024), (9, 1024), (12, 1024), (16, 1024), (18, 1024)) for N in (Np, Np - 1)]


@pytest.mark.parametrize('d,N', CASES)
def test_the_factorised_walk_runs_by_its_guard_and_keeps_the_margin_and_the_top_k(d, N):
    w = _problem(N, d, M32, 'se', seed=11 * N + d)
    e = _engine(w)
    label = 'N=%d d=%d' % (N, d)
    r, d32 = _dots(e, w['Xc'], 10, -1)
    assert r['bound_kernel'] == 'mfma32' and r['bound_fact'] is True, (label, r['bound_kernel'], r['bound_fact'], r['guard'], r['E'])
    sw = _margin(e, w, w['Xc'], r, d32, label)
    # the signs of a few weights near 0 may differ between numpy's sum and the device's: one tile either way
    assert abs(r['bound_tpos'] - _tpos_of(sw)) <= 1 and 0 <= r['bound_tpos'] <= (N + 15) // 16, (label, r['bound_tpos'], _tpos_of(sw))
    e.set_option('prune_bound', -1)
    _topk_equal(e, w['Xc'], (1, 10, 64), label)
    e.close()


@pytest.mark.parametrize('sign', [1, -1, 0])
def test_weights_of_one_sign_and_all_zero_weights(sign):
    """Under a dominant noise term K^-1 (y - bias) has the signs of y - bias; y = bias gives a = 0 and every weight 0."""
    N, d = 384, 3
    w = _problem(N, d, M32, 'se', seed=91, sn2_rel=1e4)
    rng = np.random.RandomState(5)
    w['y'] = w['bias'] + sign * (1.0 + 0.1 * rng.rand(N))
    e = _engine(w)
    label = 'sign %+d' % sign
    r, d32 = _dots(e, w['Xc'], 10, -1)
    assert r['bound_kernel'] == 'mfma32' and r['bound_fact'] is True, (label, r)
    sw = _margin(e, w, w['Xc'], r, d32, label)
    assert np.all(np.sign(sw) == sign), (label, int(np.sum(sw > 0)), int(np.sum(sw < 0)))
    assert r['bound_tpos'] == (N // 16 if sign > 0 else 0), (label, r['bound_tpos'])
    if sign == 0:
        Np = 384
        assert np.all((d32 >= 0.0) & (d32 <= 4.0 * _flush(r, Np, w['rho']))), (float(d32.min()), float(d32.max()))
    e.set_option('prune_bound', -1)
    _topk_equal(e, w['Xc'], (1, 10, 64), label)
    e.close()


def test_a_scaled_weight_outside_fp32_hands_the_walk_to_the_unfactorised_form():
    """Every w normal in fp32, some w' = w r_i below 2^-126: the fp32 kernel runs by its guards, unfactorised."""
    N, d, k = 1024, 2, 10
    w = _problem(N, d, M32, 'se', seed=61)
    w['y'], w['bias'] = w['y'] - w['bias'], 0.0
    e = _engine(w)
    a0 = np.abs(_signed_weights(e, w))
    e.close()
    w['y'] = w['y'] * (1.02 * W_MIN / a0[a0 > 0.0].min())       # the smallest weight just inside the normal range
    e = _engine(w)
    sw = _signed_weights(e, w)
    Xs = w['X'] / w['ell']
    cen = 0.5 * Xs.min(0) + 0.5 * Xs.max(0)
    ri = np.exp(-0.5 * ((Xs - cen) ** 2).sum(1))
    assert np.all((sw == 0.0) | (np.abs(sw) >= W_MIN)) and np.any((sw != 0.0) & (np.abs(sw) * ri < W_MIN)), (np.abs(sw).min(), (np.abs(sw) * ri).min())
    rg, dg = _dots(e, w['Xc'], k, -1)
    assert rg['bound_kernel'] == 'mfma32' and rg['bound_fact'] is False and 0.0 < rg['E'] <= E_MAX, rg
    _margin(e, w, w['Xc'], rg, dg, "subnormal w'")
    r0, d0 = _dots(e, w['Xc'], k, -1, fact=0)
    assert r0['bound_kernel'] == 'mfma32' and r0['bound_fact'] is False and np.array_equal(dg, d0)
    e.close()


def test_radii_beyond_the_range_guard_keep_the_unfactorised_form_under_the_forced_kernel():
    """d = 1, length scale 0.02, observations and candidates over [0, 1]: R_x = R_z = 25, L R_x R_z = 900 > 120 while E < 2^-10 (at
    these N the fp64 guard declines long before: only the forced kernel walks here).  With a longer length scale the same handle's
    forced kernel takes the factorised form."""
    N, M, k = 300, 3 * G + 77, 10
    for ell, fact in ((0.02, False), (0.5, True)):
        w = _problem(N, 1, M, 'se', seed=33)
        w['ell'] = np.array([ell])
        w['X'][0], w['X'][1] = 0.0, 1.0
        e = _engine(w)
        r2, d2 = _dots(e, w['Xc'], k, 2)
        x = LOG2E * (0.5 / ell) * np.max(np.abs(w['Xc'] - 0.5)) / ell
        assert r2['bound_kernel'] == 'mfma32' and r2['bound_fact'] is fact and r2['E'] <= E_MAX and (x > 120.0) != fact, (ell, x, r2)
        assert (r2['guard'] > 384) != fact
        _margin(e, w, w['Xc'], r2, d2, 'forced ell=%g' % ell)
        r0, d0 = _dots(e, w['Xc'], k, 2, fact=0)
        assert r0['bound_fact'] is False and (np.array_equal(d2, d0) != fact), ell
        e.close()


@pytest.mark.parametrize('fact', [1, 0])
def test_a_candidate_on_an_observation_a_nan_one_and_a_far_one(fact):
    M, k = 3 * G + 77, 10
    w = _problem(300, 3, M, 'se', seed=51)
    Z = w['Xc'].copy()
    Z[5] = w['X'][7]
    Z[9, 1] = np.nan
    Z[11] = 50.0                           # 100 length scales away: E > 2^-10, no finite margin -- and no factorised walk
    e = _engine(w)
    e.set_option('prune_bound', 2)
    e.set_option('bound_fact', fact)
    r = check_sweep(e, w, Z, k, prune=1, label='edges bound=2 fact=%d' % fact)
    d32 = e.prune_dots()
    assert r['bound_kernel'] == 'mfma32' and r['bound_fact'] is False
    assert np.isnan(d32[9]) and np.isnan(r['ub_kept'][9]) and (9 in r['seed_idx'] or 9 in r['idx'])
    assert np.isfinite(d32[5]) and 0.0 <= d32[11] <= 1e-30 * (w['rho'] * r['S'] + 384)
    # without the far one the guards pass: the factorised walk where the option allows, the NaN kept, the on-observation dot finite
    Z[11] = w['Xc'][11]
    r = check_sweep(e, w, Z, k, prune=1, label='edges near bound=2 fact=%d' % fact)
    d32 = e.prune_dots()
    assert r['bound_kernel'] == 'mfma32' and r['bound_fact'] is (fact == 1)
    assert np.isnan(d32[9]) and np.isnan(r['ub_kept'][9]) and (9 in r['seed_idx'] or 9 in r['idx'])
    assert np.isfinite(d32[5])
    e.set_option('bound_fact', 1)
    _margin(e, w, Z, r, d32, 'edges near fact=%d' % fact)
    e.close()


def test_the_ensemble_sweep_reports_each_members_form():
    from test_gpu_ens_prune import _ensemble, _same, _sweep
    p, engines = _ensemble('se_n3')
    try:
        plain = _sweep(p, engines, p['Z'], 10, 0)
        for e in engines:
            e.set_option('prune_bound', 2)
        pruned = _sweep(p, engines, p['Z'], 10, 1)
        assert _same(plain, pruned) and pruned[3]['path'] == 'pruned'
        assert np.array_equal(pruned[3]['bound_fact'], np.ones(3)), pruned[3]['bound_fact']
        engines[1].set_option('bound_fact', 0)
        mixed = _sweep(p, engines, p['Z'], 10, 1)
        assert _same(plain, mixed) and np.array_equal(mixed[3]['bound_fact'], [1.0, 0.0, 1.0]), mixed[3]['bound_fact']
        for e in engines:
            e.set_option('prune_bound', 1)
        ref = _sweep(p, engines, p['Z'], 10, 1)
        assert _same(plain, ref) and np.array_equal(ref[3]['bound_fact'], np.zeros(3))
    finally:
        for e in engines:
            e.set_option('prune_bound', -1)
            e.set_option('bound_fact', 1)
