"""tests/sampler_ref.py, the numpy reference the GPU pins of the sampler's small kernels are held to, is itself pinned here without a GPU: the generator
against the published Random123 known answers, the schedule coefficients and the index rule against the oracle / torch, the step and decode algebra
against the oracle's sample_p_zs_given_zt / sample_p_xh_given_z0 on a tape draw."""
import numpy as np
import pytest
import torch

import sampler_ref as R
from oracle import gcdm_oracle as O

# Random123 kat_vectors, philox4x32 with 10 rounds: counter, key, output (words in counter order)
KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF), (0xFFFFFFFF, 0xFFFFFFFF), (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    assert tuple(R.philox4x32_10(counter, key)) == want
    got = R.philox4x32_10([np.array([c, c], dtype=np.uint64) for c in counter], [np.uint64(k) for k in key])      # the vectorised form
    assert [int(w[1]) for w in got] == list(want) and all(w.dtype == np.uint64 for w in got)


def test_philox_normal_follows_the_documented_contract():
    """counter {node, draw, col >> 1, tag}, key {seed low, seed high}; the two columns of a pair share one block: cosine lane, then sine lane."""
    seed, draw, node = (0xDEADBEEF << 32) | 0x12345678, R.DRAW_INIT, 41
    for col in (0, 1, 6, 7):
        w = R.philox4x32_10((node, draw, col >> 1, R.COUNTER_TAG), (0x12345678, 0xDEADBEEF))
        u1 = (np.float32(w[0] >> 8) + np.float32(0.5)) * np.float32(2.0 ** -24)
        u2 = (np.float32(w[1] >> 8) + np.float32(0.5)) * np.float32(2.0 ** -24)
        r, ang = np.sqrt(-2.0 * np.log(np.float64(u1))), 2.0 * np.pi * np.float64(u2)
        assert float(R.philox_normal(seed, draw, node, col)) == (r * np.sin(ang) if col & 1 else r * np.cos(ang))
    tab = R.philox_table(seed, 3, 70, 9, node_base=37)
    assert tab.shape == (70, 9) and tab.dtype == np.float64
    assert tab[5, 4] == float(R.philox_normal(seed, 3, 42, 4)) and tab[69, 8] == float(R.philox_normal(seed, 3, 106, 8))
    # pairs, draws, nodes and seeds are all distinct streams
    flat = np.concatenate([R.philox_table(seed, 3, 70, 9).ravel(), R.philox_table(seed, 4, 70, 9).ravel(), R.philox_table(seed + 1, 3, 70, 9).ravel()])
    assert len(np.unique(flat)) == flat.size
    assert abs(flat.mean()) < 0.1 and abs(flat.std() - 1.0) < 0.1


def test_uniform_edges_give_finite_normals():
    m = np.array([0, 2 ** 23 - 1, 2 ** 23, 2 ** 24 - 2, 2 ** 24 - 1], dtype=np.uint64)
    u = R.uniform24(m << np.uint64(8) | np.uint64(0xFF))
    assert u.dtype == np.float32 and (u > 0).all() and (u <= 1).all()
    assert u[0] == np.float32(2.0 ** -25) and u[-1] == np.float32(1.0) and u[-2] < 1.0
    assert u[2] == np.float32(0.5)                        # 2^23 + 0.5 is a tie in fp32: rounds to even
    for col in (0, 1):
        for w1 in m:
            z = R.box_muller(m << np.uint64(8), np.full(5, int(w1) << 8, dtype=np.uint64), col)
            assert np.isfinite(z).all() and np.abs(z).max() <= 5.9 and z[-1] == 0.0        # |r| <= sqrt(50 ln 2) = 5.887; u1 = 1 gives exactly 0


def test_fp64_coefficients_equal_the_oracle():
    ocfg = O.OracleConfig()
    gam32 = O.gamma_table(ocfg)
    gam = gam32.double()
    T = ocfg.num_timesteps
    for s, n in [(0, 1000), (1, 1000), (499, 1000), (999, 1000), (1, 400), (399, 400), (3, 7), (0, 1)]:
        sv, tv = torch.tensor([[s / n]], dtype=torch.float32), torch.tensor([[(s + 1) / n]], dtype=torch.float32)
        gs, gt = O.gamma_at(gam, sv, T), O.gamma_at(gam, tv, T)
        s2, sts, ats = O.sigma_and_alpha_t_given_s(gt, gs)
        sig_s, sig_t = torch.sqrt(torch.sigmoid(gs)), torch.sqrt(torch.sigmoid(gt))
        want = [ats.item(), (s2 / ats / sig_t).item(), (sts * sig_s / sig_t).item()]
        g2 = R.gamma_pair(gam32.numpy(), s, s + 1, n)
        assert (float(g2[0]), float(g2[1])) == (gs.item(), gt.item())
        np.testing.assert_allclose(R.step_coeffs(*g2), want, rtol=1e-13)
        np.testing.assert_allclose(R.jump_coeffs(*g2), [ats.item(), sts.item()], rtol=1e-13)
        np.testing.assert_allclose(R.noising_coeffs(g2[0]), [torch.sqrt(torch.sigmoid(-gs)).item(), sig_s.item()], rtol=1e-13)
        # the fp32 evaluation is torch's fp32 evaluation to a few units in the last place of the terms (libm against torch's vectorised functions)
        s2f, stsf, atsf = O.sigma_and_alpha_t_given_s(gt.float(), gs.float())
        c32 = R.step_coeffs(*g2, dtype=np.float32)
        assert all(isinstance(v, np.float32) for v in c32)
        np.testing.assert_allclose(c32[0], atsf.item(), rtol=64 * 2.0 ** -24)
        np.testing.assert_allclose(c32[2], (stsf * torch.sqrt(torch.sigmoid(gs.float())) / torch.sqrt(torch.sigmoid(gt.float()))).item(), rtol=1e-3, atol=1e-7)
    g0 = gam[0]
    np.testing.assert_allclose(R.final_coeffs(gam32.numpy()[0]), [(1.0 / torch.sqrt(torch.sigmoid(-g0))).item(), torch.sqrt(torch.sigmoid(g0)).item(),
                                                                torch.exp(0.5 * g0).item()], rtol=1e-13)


@pytest.mark.parametrize("s,num_steps", [(1, 400), (3, 400), (399, 400), (0, 1), (3, 7)])
def test_index_rule_is_torch_round_on_fp32(s, num_steps):
    for T in (1000, 500, 7):
        for k in (s, s + 1):
            t = torch.tensor(k, dtype=torch.float32) / torch.tensor(num_steps, dtype=torch.float32)
            want = int(torch.round(t * T).long().clamp(0, T))
            assert R.timestep_index(np.float32(k) / np.float32(num_steps), T) == want
    assert R.timestep_index(np.float32(1) / np.float32(400), 1000) == 2 and R.timestep_index(np.float32(3) / np.float32(400), 1000) == 8      # 2.5 -> 2, 7.5 -> 8
    assert R.timestep_index(np.float32(-1.0), 10) == 0 and R.timestep_index(np.float32(2.0), 10) == 10


def _case(num_nodes, F, seed):
    nn_ = torch.tensor(num_nodes)
    bi = O.num_nodes_to_batch_index(nn_)
    N = len(bi)
    mask = torch.ones(N, dtype=torch.bool)
    z = torch.randn((N, 3 + F), generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 0.3
    z[:, :3] = O.centralize(z[:, :3], bi, len(nn_), mask)
    tape = O.TapeNoise(seed + 1)
    raw = torch.cat((tape(N, 3), tape(N, F)), dim=-1)
    return nn_, bi, mask, z, raw


@pytest.mark.parametrize("fix_noise", [False, True])
def test_step_mode_equals_the_oracles_algebra(fix_noise):
    """sample_p_zs_given_zt in fp64 with the network's output given (zero, and a random one) on a tape draw."""
    ocfg = O.OracleConfig()
    F = ocfg.num_node_scalar_features
    nn_, bi, mask, z, raw = _case([1, 2, 6, 19], F, 5)
    gam = O.gamma_table(ocfg)
    noff = R.offsets(nn_.tolist())
    for eps in (torch.zeros_like(z), torch.randn(z.shape, generator=torch.Generator().manual_seed(9), dtype=torch.float64)):
        for s, n in [(0, 1000), (499, 1000), (3, 7)]:
            sv, tv = float(np.float32(s) / np.float32(n)), float(np.float32(s + 1) / np.float32(n))
            want, _ = O.sample_p_zs_given_zt({}, ocfg, gam, sv, tv, z, bi, len(nn_), mask, None, O.TapeNoise(6), eps_override=eps, fix_noise=fix_noise)
            gm = R.noise_mean(raw.numpy()) if fix_noise else None
            got = R.mode_step(z.numpy(), eps.numpy(), raw.numpy(), noff, R.step_coeffs(*R.gamma_pair(gam.numpy(), s, s + 1, n)), gmean=gm)
            np.testing.assert_allclose(got, want.numpy(), rtol=0, atol=1e-12 * max(1.0, want.abs().max().item()))
            got32 = R.mode_step(z.numpy(), eps.numpy(), raw.numpy(), noff, R.step_coeffs(*R.gamma_pair(gam.numpy(), s, s + 1, n), dtype=np.float32), gmean=gm,
                                dtype=np.float32)
            assert got32.dtype == np.float32 and np.abs(got32 - got).max() <= 1e-4 * max(1.0, np.abs(got).max())


@pytest.mark.parametrize("shift", [0.0, 0.01, 0.75])
def test_final_mode_equals_the_oracles_algebra(shift, monkeypatch):
    """sample_p_xh_given_z0 + the drift decision of mol_gen_sample in fp64, the network replaced by a fixed output."""
    ocfg = O.OracleConfig()
    F = ocfg.num_node_scalar_features
    nn_, bi, mask, z, raw = _case([1, 2, 6, 19], F, 7)
    z[bi == 2, 0] += shift
    B = len(nn_)
    eps = torch.randn(z.shape, generator=torch.Generator().manual_seed(11), dtype=torch.float64) * 0.1
    monkeypatch.setattr(O, "dynamics_forward", lambda *a, **k: eps)
    gam = O.gamma_table(ocfg)
    x, one_hot, charges = O.sample_p_xh_given_z0({}, ocfg, gam, z, bi, B, mask, None, O.TapeNoise(8))
    drift = torch.zeros(B, 3, dtype=x.dtype).index_add_(0, bi, x).abs().max().item() > 5e-2
    if drift:
        x = O.centralize(x, bi, B, mask)
    norm = R.Norm(ocfg.num_atom_types, ocfg.include_charges, ocfg.norm_values, (0.0, 0.0, 0.0))
    got = R.mode_final(z.numpy(), eps.numpy(), raw.numpy(), R.offsets(nn_.tolist()), R.final_coeffs(gam.numpy()[0]), norm)
    assert got.drift == drift
    # 1 atom: sum = shift-free x of one node; drift only through the shifted molecule or the noise -- both sides of 5e-2 are met over the parameters
    np.testing.assert_allclose(got.x, x.numpy(), rtol=0, atol=1e-12)
    assert np.array_equal(got.one_hot, one_hot.numpy()) and np.array_equal(got.charge, charges.numpy()[:, 0])
    off = R.mode_final(z.numpy(), eps.numpy(), raw.numpy(), R.offsets(nn_.tolist()), R.final_coeffs(gam.numpy()[0]), norm, cog_fix=False)
    np.testing.assert_allclose(off.x, got.cont[:, :3], rtol=0, atol=0)


def test_network_free_modes_equal_the_oracle():
    ocfg = O.OracleConfig()
    F = ocfg.num_node_scalar_features
    nn_, bi, mask, z, raw = _case([1, 2, 6, 19], F, 13)
    B = len(nn_)
    noff = R.offsets(nn_.tolist())
    gam = O.gamma_table(ocfg)
    norm = R.Norm(ocfg.num_atom_types, ocfg.include_charges, ocfg.norm_values, (0.0, 0.0, 0.0))
    np.testing.assert_allclose(R.unnormalize(z.numpy(), norm), O.unnormalize_z(ocfg, z, mask).numpy(), rtol=0, atol=1e-13)
    np.testing.assert_allclose(R.encode(R.unnormalize(z.numpy(), norm), norm), z.numpy(), rtol=0, atol=1e-13)
    x_n, h_n = O.normalize(ocfg, z[:, :3], z[:, 3:3 + ocfg.num_atom_types], mask)
    np.testing.assert_allclose(R.encode(z.numpy(), norm)[:, :3 + ocfg.num_atom_types], torch.cat((x_n, h_n), dim=-1).numpy(), rtol=0, atol=1e-13)
    assert R.mean_zero_error(z.numpy()[:, :3], noff) == pytest.approx(O.assert_mean_zero_with_mask(z[:, :3], bi, B), abs=1e-15)
    # q(z_t | z_s) with its projection (mode 4), and the init draw (mode 1)
    for s, t, n in [(0, 1, 6), (2, 4, 6), (1, 400, 400)]:
        sv, tv = float(np.float32(s) / np.float32(n)), float(np.float32(t) / np.float32(n))
        want = O.sample_p_zt_given_zs(ocfg, gam, z, sv, tv, bi, B, mask, O.TapeNoise(14))
        got = R.mode_jump(z.numpy(), None, raw.numpy(), noff, R.jump_coeffs(*R.gamma_pair(gam.numpy(), s, t, n)))
        np.testing.assert_allclose(got, want.numpy(), rtol=0, atol=1e-12)
    want = O.sample_combined_noise(O.TapeNoise(14), bi, B, mask, F, torch.float64)
    np.testing.assert_allclose(R.mode_init(None, None, raw.numpy(), noff), want.numpy(), rtol=0, atol=1e-13)
    assert np.array_equal(R.mode_init(None, None, raw.numpy(), noff)[0, :3], np.zeros(3))            # one node: the CoM-free x-noise is exactly 0
    want = O.sample_combined_noise(O.TapeNoise(14), bi, B, mask, F, torch.float64, fix_noise=True)
    np.testing.assert_allclose(R.mode_init(None, None, raw.numpy(), noff, gmean=R.noise_mean(raw.numpy())), want.numpy(), rtol=0, atol=1e-13)
    # inpainting: centring on the fixed nodes and the combine
    fixed = torch.zeros(len(bi), dtype=torch.bool)
    fixed[[1, 3, 4, 7]] = True
    fixed[9:] = torch.rand(len(bi) - 9, generator=torch.Generator().manual_seed(3)) < 0.4
    fm = O._fixed_mean(z[:, :3], fixed, bi, B)
    np.testing.assert_allclose(R.fixed_mean(z.numpy()[:, :3], fixed.numpy(), noff), fm[bi].numpy(), rtol=0, atol=1e-13)
    cen = R.inpaint_center(z.numpy(), fixed.numpy(), noff)
    np.testing.assert_allclose(cen[:, :3], (z[:, :3] - fm[bi]).numpy(), rtol=0, atol=1e-13)
    assert np.array_equal(cen[:, 3:], z.numpy()[:, 3:]) and np.array_equal(cen[:1], z.numpy()[:1])        # molecule 0 has no fixed node: shift 0
    zu = raw.double().numpy()
    comb = R.inpaint_combine(z.numpy(), zu, fixed.numpy(), noff)
    assert np.array_equal(comb[~fixed.numpy()], zu[~fixed.numpy()]) and np.array_equal(comb[fixed.numpy(), 3:], z.numpy()[fixed.numpy(), 3:])
    for b in range(1, B):
        sel = fixed.numpy() & (bi.numpy() == b)
        np.testing.assert_allclose(comb[sel, :3].mean(0), zu[sel, :3].mean(0), rtol=0, atol=1e-13)      # the fixed nodes take the unknown part's CoM
