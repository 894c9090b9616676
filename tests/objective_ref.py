"""The fused diffusion objective (include/gcdm_objective.h) restated in torch on the CPU, one thread, in fp64 or fp32, entry by entry with the
C ABI's arguments.  Every function also returns `mag`: per output the sum of the absolute values of the terms that were added up to give it,
the Sigma |terms| of the project's bar  |got - ref64| <= M |ref32 - ref64| + 8 * 2^-24 * Sigma |terms|.

`mutant=` applies one wrong reading of the header to the restatement (MUTANTS); tests/test_objective_cpu.py shows that the bar rejects each
when it is applied to the fp32 run."""
import math

import torch

TRAIN_VLB, EVAL, TRAIN_L2 = 0, 1, 2
MUTANTS = ("s_index_clamped", "com_over_all_rows", "no_logsumexp", "epsilon_inside_erf", "no_one_minus_t_is_zero", "denominator_without_max_nodes",
           "integer_mass_ignores_mask")
TERMS = ("delta_log_px", "error_t", "SNR_weight", "loss_0_x", "loss_0_h", "neg_log_constants", "kl_prior", "log_pN", "eps_hat_x", "eps_hat_h")
U = 2.0 ** -24


def offsets_of(num_nodes):
    nn_ = torch.as_tensor(num_nodes, dtype=torch.int64)
    return torch.cat([torch.zeros(1, dtype=torch.int64), nn_.cumsum(0)]).to(torch.int32)


def _bi(off):
    off = off.long()
    return torch.repeat_interleave(torch.arange(len(off) - 1), off[1:] - off[:-1])


def _seg(v, bi, B):
    return torch.zeros((B,) + tuple(v.shape[1:]), dtype=v.dtype).index_add_(0, bi, v)


def gamma_indices(t_int, T, mutant=None):
    """fp32 in every run: the index rule is part of the contract, not of the arithmetic."""
    t = t_int.long()
    it = torch.round((t / T).float() * T).long()
    is_ = torch.round(((t - 1) / T).float() * T).long()
    is_ = is_.clamp(min=0) if mutant == "s_index_clamped" else torch.where(is_ < 0, is_ + T + 1, is_)
    return it, is_


def _sig(g):
    return torch.sqrt(torch.sigmoid(g))


def prepare(x, one_hot, charges, mask, off, t_int, gamma, log_pn, nv, nb, eps_raw, eps_raw_0, nf, ic, T, mode, center_x=False,
            dtype=torch.float64, mutant=None):
    torch.set_num_threads(1)
    c = lambda v: None if v is None else v.to(dtype)          # noqa: E731
    B, N, D = len(off) - 1, x.shape[0], 3 + nf + ic
    bi = _bi(off)
    m = torch.ones(N, dtype=dtype) if mask is None else (mask != 0).to(dtype)
    mu = m.unsqueeze(-1)
    g = gamma.to(dtype)
    it, is_ = gamma_indices(t_int, T, mutant)
    flags = 0
    g_t, g_s, g_T, g_0 = g[it], g[is_], g[T], g[0]
    cnt = _seg(m, bi, B)
    mcom = torch.ones_like(m) if mutant == "com_over_all_rows" else m
    ccom = _seg(mcom, bi, B)
    xs = c(x)
    xmag = xs.abs()
    if center_x:
        xmag = xmag + (_seg(xmag, bi, B) / cnt.unsqueeze(-1))[bi] * mu
        xs = xs - (_seg(xs, bi, B) / cnt.unsqueeze(-1))[bi] * mu
    cols = [xs / nv[0], (c(one_hot) - nb[1]) / nv[1] * mu]
    if ic:
        cols.append(((c(charges).reshape(-1) - nb[2]) / nv[2] * m).unsqueeze(-1))
    xh = torch.cat(cols, dim=-1)
    out, mag = {"xh": xh}, {"xh": torch.cat([xmag / nv[0], xh[:, 3:].abs()], dim=-1)}

    def project(raw):
        e = c(raw) * mu
        ex = c(raw)[:, :3] if mutant == "com_over_all_rows" else e[:, :3]
        mean = _seg(ex, bi, B) / ccom.unsqueeze(-1)
        amean = _seg(ex.abs(), bi, B) / ccom.unsqueeze(-1)
        ep = torch.cat([e[:, :3] - mean[bi] * mu, e[:, 3:]], dim=-1)
        em = torch.cat([e[:, :3].abs() + amean[bi] * mu, e[:, 3:].abs()], dim=-1)
        return ep, em

    eps_t, me = project(eps_raw)
    a_t, s_t = _sig(-g_t)[bi].unsqueeze(-1), _sig(g_t)[bi].unsqueeze(-1)
    out.update(eps_t=eps_t, z_t=a_t * xh + s_t * eps_t, t_node=(t_int.long() / T).to(torch.float32).to(dtype)[bi])
    mag.update(eps_t=me, z_t=a_t * mag["xh"] + s_t * me, t_node=out["t_node"].abs())
    if mode == EVAL:
        eps_0, m0 = project(eps_raw_0)
        out.update(eps_0=eps_0, z_0=_sig(-g_0) * xh + _sig(g_0) * eps_0)
        mag.update(eps_0=m0, z_0=_sig(-g_0) * mag["xh"] + _sig(g_0) * m0)
    sub = (cnt - 1) * 3
    mol = torch.zeros(B, 8, dtype=dtype)
    mm = torch.zeros(B, 8, dtype=dtype)
    mol[:, 0] = -sub * math.log(float(nv[0]))
    mol[:, 1] = -(sub * (-0.5 * g_0 - 0.5 * math.log(2 * math.pi)))
    muT = _sig(-g_T) * xh
    qx, qh = _seg((muT[:, :3] ** 2).sum(-1), bi, B), _seg((muT[:, 3:] ** 2 * mu).sum(-1), bi, B)
    sT = _sig(g_T)
    lg = torch.log(1.0 / sT)
    mol[:, 2] = (sub * lg + 0.5 * (sub * sT ** 2 + qx) - 0.5 * sub) + (lg + 0.5 * (sT ** 2 + qh) - 0.5)
    mm[:, 2] = sub * lg.abs() + 0.5 * (sub * sT ** 2 + qx) + 0.5 * sub + lg.abs() + 0.5 * (sT ** 2 + qh) + 0.5
    mol[:, 3] = torch.exp(-(g_s - g_t)) - 1
    mm[:, 3] = torch.exp(-(g_s - g_t)) + 1
    mol[:, 4] = (t_int.long() == 0).to(dtype)
    mol[:, 5] = cnt
    idx = cnt.long()
    lp = torch.full((B,), float("nan"), dtype=dtype)
    ok = (idx >= 0) & (idx < len(log_pn))
    lp[ok] = log_pn.to(dtype)[idx[ok]]
    if torch.isnan(lp).any():
        flags |= 2
    mol[:, 6] = lp
    mol[:, 7] = g_t
    for k in (0, 1, 4, 5, 6, 7):
        mm[:, k] = mol[:, k].abs()
    out["mol"], mag["mol"] = mol, mm
    out["flags"] = flags
    return out, mag


def _mass(centre, width, mutant=None):
    cdf = lambda v: 0.5 * (1.0 + torch.erf(v * (0.5 ** 0.5)))          # noqa: E731
    if mutant == "epsilon_inside_erf":
        return torch.log(cdf((centre + 0.5) / width + 1e-10) - cdf((centre - 0.5) / width))
    return torch.log(cdf((centre + 0.5) / width) - cdf((centre - 0.5) / width) + 1e-10)


def mass_argument(prep, off, gamma, nv, nb, nf, ic, mode):
    """cdf difference of every mass the terms take a log of (unmasked rows): the tests keep it clear of the 1e-10 epsilon."""
    dtype = prep["xh"].dtype
    bi = _bi(off)
    sig0 = _sig(gamma.to(dtype)[0].expand(len(off) - 1) if mode == EVAL else prep["mol"][:, 7])[bi].unsqueeze(-1)
    z = prep["z_0"] if mode == EVAL else prep["z_t"]
    cdf = lambda v: 0.5 * (1.0 + torch.erf(v * (0.5 ** 0.5)))          # noqa: E731
    cen = z[:, 3:3 + nf] * nv[1] + nb[1] - 1.0
    d = [cdf((cen + 0.5) / (sig0 * nv[1])) - cdf((cen - 0.5) / (sig0 * nv[1]))]
    if ic:
        ci = torch.round(prep["xh"][:, -1:] * nv[2] + nb[2]) - (z[:, -1:] * nv[2] + nb[2])
        d.append(cdf((ci + 0.5) / (sig0 * nv[2])) - cdf((ci - 0.5) / (sig0 * nv[2])))
    return torch.cat(d, dim=-1)


def terms(net_out, net_out_0, prep, mask, off, gamma, nv, nb, nf, ic, T, mode, dtype=torch.float64, mutant=None):
    torch.set_num_threads(1)
    B, D = len(off) - 1, 3 + nf + ic
    bi = _bi(off)
    N = len(bi)
    m = torch.ones(N, dtype=dtype) if mask is None else (mask != 0).to(dtype)
    mu = m.unsqueeze(-1)
    mol = prep["mol"].to(dtype)
    t0 = mol[:, 4]
    no = net_out.to(dtype)
    ev = mode == EVAL
    eps, net, z = (prep["eps_0"], net_out_0.to(dtype), prep["z_0"]) if ev else (prep["eps_t"], no, prep["z_t"])
    sig0 = _sig(gamma.to(dtype)[0] if ev else mol[:, 7])
    sig0 = (sig0.expand(B) if sig0.dim() == 0 else sig0)[bi].unsqueeze(-1)
    xh = prep["xh"]
    err = _seg(((prep["eps_t"] - no) ** 2).sum(-1), bi, B)          # over ALL rows, as the reference (tests/golden/train_full_qm9mask.npz)
    l0x = 0.5 * _seg((((eps[:, :3] - net[:, :3]) ** 2) * mu).sum(-1), bi, B)
    lp = _mass(z[:, 3:3 + nf] * nv[1] + nb[1] - 1.0, sig0 * nv[1], mutant)
    if mutant != "no_logsumexp":
        lp = lp - torch.logsumexp(lp, dim=-1, keepdim=True)
    w = (xh[:, 3:3 + nf] * nv[1] + nb[1]) * mu
    lph = _seg((lp * w).sum(-1), bi, B)
    mph = _seg((lp * w).abs().sum(-1), bi, B)
    if ic:
        hi = torch.round(xh[:, -1:] * nv[2] + nb[2])
        mi = _mass(hi - (z[:, -1:] * nv[2] + nb[2]), sig0 * nv[2], mutant) * (1.0 if mutant == "integer_mass_ignores_mask" else mu)
        lph = lph + _seg(mi.sum(-1), bi, B)
        mph = mph + _seg(mi.abs().sum(-1), bi, B)
    l0h = -lph
    if not ev:
        if mutant != "no_one_minus_t_is_zero":
            err = err * (1 - t0)
        l0x, l0h, mph = l0x * t0, l0h * t0, mph * t0
    rows = (off[1:] - off[:-1]).to(dtype).clamp(min=1)
    l2 = mode == TRAIN_L2
    out = torch.zeros(B, 10, dtype=dtype)
    out[:, 0] = 0 if l2 else mol[:, 0]
    out[:, 1] = err
    out[:, 2] = 1 if l2 else mol[:, 3]
    out[:, 3], out[:, 4] = l0x, l0h
    out[:, 5] = 0 if l2 else mol[:, 1]
    out[:, 6], out[:, 7] = mol[:, 2], mol[:, 6]
    out[:, 8] = _seg(no[:, :3].abs().mean(-1), bi, B) / rows
    out[:, 9] = _seg(no[:, 3:].abs().mean(-1), bi, B) / rows
    mag = out.abs()
    mag[:, 4] = mph
    return out, mag


def reduce(mol, terms_, D, T, mode, by_max, dtype=torch.float64, mutant=None):
    t = terms_.to(dtype)
    B = t.shape[0]
    if mode == TRAIN_L2:
        n = mol[:, 5].to(dtype)
        den = D * (n.max() if (by_max and mutant != "denominator_without_max_nodes") else n)
        ct, c0 = 0.5 / den * torch.ones(B, dtype=dtype), 1.0 / den * torch.ones(B, dtype=dtype)
        loss_t, loss_0 = 0.5 * (t[:, 1] / den), t[:, 3] / den + t[:, 4]
        m0 = (t[:, 3] / den).abs() + t[:, 4].abs()
    else:
        ct, c0 = T * 0.5 * t[:, 2], torch.ones(B, dtype=dtype)
        loss_t, loss_0 = ct * t[:, 1], t[:, 3] + t[:, 4] + t[:, 5]
        m0 = t[:, 3].abs() + t[:, 4].abs() + t[:, 5].abs()
    nll = loss_t + loss_0 + t[:, 6] - t[:, 0] - t[:, 7]
    mn = loss_t.abs() + m0 + t[:, 6].abs() + t[:, 0].abs() + t[:, 7].abs()
    cols = (nll, loss_t, t[:, 2], loss_0, t[:, 6], t[:, 0], t[:, 5], t[:, 7], t[:, 8], t[:, 9])
    means = torch.zeros(16, dtype=dtype)
    mmag = torch.zeros(16, dtype=dtype)
    for k, v in enumerate(cols):
        means[k], mmag[k] = v.mean(), v.abs().mean()
    mmag[0] = mn.mean()
    return nll, means, torch.stack([ct, c0], dim=-1), {"nll": mn, "means": mmag}


def bwd(g_error_t, g_loss_0_x, g_nll, g_loss, net_out, eps_t, mask, off, mol, coef, dtype=torch.float64):
    """The closed form the kernel uses."""
    B = len(off) - 1
    bi = _bi(off)
    z = torch.zeros(B, dtype=dtype)
    G = (z if g_nll is None else g_nll.to(dtype).expand(B)) + (0 if g_loss is None else g_loss.to(dtype) / B)
    Gt = (z if g_error_t is None else g_error_t.to(dtype).expand(B)) + G * coef[:, 0].to(dtype)
    G0 = (z if g_loss_0_x is None else g_loss_0_x.to(dtype).expand(B)) + G * coef[:, 1].to(dtype)
    t0 = mol[:, 4].to(dtype)
    m = torch.ones(len(bi), dtype=dtype) if mask is None else (mask != 0).to(dtype)
    df = eps_t.to(dtype) - net_out.to(dtype)
    d = (-2 * (1 - t0) * Gt)[bi].unsqueeze(-1) * df
    d[:, :3] += (-(t0 * G0))[bi].unsqueeze(-1) * df[:, :3] * m.unsqueeze(-1)
    return d


def run(inp, net_out, net_out_0=None, by_max=False, dtype=torch.float64, mutant=None):
    """prepare + terms + reduce on one input dictionary (the keyword arguments of `prepare` but dtype / mutant)."""
    prep, pm = prepare(**inp, dtype=dtype, mutant=mutant)
    a = inp
    tr, tm = terms(net_out, net_out_0, prep, a["mask"], a["off"], a["gamma"], a["nv"], a["nb"], a["nf"], a["ic"], a["T"], a["mode"], dtype, mutant)
    nll, means, coef, rm = reduce(prep["mol"], tr, 3 + a["nf"] + a["ic"], a["T"], a["mode"], by_max, dtype, mutant)
    return dict(prep=prep, terms=tr, nll=nll, means=means, coef=coef), dict(prep=pm, terms=tm, **rm)


def bar_ok(got, r32, r64, mag, M=4.0):
    """-> (ok, worst factor): |got - r64| <= M |r32 - r64| + 8 * 2^-24 * mag, element-wise; the factor is the M that would just pass."""
    got, r32, r64, mag = (torch.as_tensor(v).double() for v in (got, r32, r64, mag))
    same_nan = torch.isnan(got) == torch.isnan(r64)
    fin = ~torch.isnan(r64)
    err = (got - r64).abs()[fin]
    slack = 8 * U * mag[fin]
    own = (r32 - r64).abs()[fin]
    ok = bool(same_nan.all()) and bool((err <= M * own + slack).all())
    over = (err - slack).clamp(min=0)
    fac = torch.where(over > 0, over / own.clamp(min=1e-300), torch.zeros_like(over))
    return ok, (float(fac.max()) if fac.numel() else 0.0)
