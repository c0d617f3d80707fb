"""Long-double reference of the pathwise samples (gogp_amd/pathwise.py, csrc/pathwise.hip): the similarity of radial terms and
its derivative in the first argument, and the random features with theirs.  A term is a dict(kind, c, il) with il the
NDim inverse lengths; terms_of(gp) reads them off a GP at its ThetaSimil."""
import numpy as np

from gogp_amd.kernel import K_MATERN32, K_MATERN52_TEXTBOOK, K_NORMAL

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)


def terms_of(gp):
    th = np.asarray(gp.ThetaSimil, float)
    return [dict(kind=t.kind, c=th[t.scale_idx] if t.scale_idx >= 0 else 1.0,
                 il=1.0 / (th[t.len_idx:t.len_idx + gp.NDim] if t.ard else np.full(gp.NDim, th[t.len_idx])))
            for t in gp.Simil.terms]


def kern(terms, Z, X, deriv=False):
    """k(Z, X) (m, n), or with deriv dk(z_i, x_j)/dz_d (m, n, NDim)."""
    diff = Z.astype(LD)[:, None, :] - X.astype(LD)[None, :, :]
    out = np.zeros(diff.shape if deriv else diff.shape[:2], LD)
    for t in terms:
        il = np.asarray(t["il"], LD)
        r2 = ((diff * il) ** 2).sum(-1)
        r = np.sqrt(r2)
        s3, s5 = np.sqrt(LD(3)), np.sqrt(LD(5))
        if t["kind"] == K_NORMAL:
            f = np.exp(-r2 / 2)
            df = -f / 2
        elif t["kind"] == K_MATERN32:
            f, df = (1 + s3 * r) * np.exp(-s3 * r), -LD(3) / 2 * np.exp(-s3 * r)
        else:
            assert t["kind"] == K_MATERN52_TEXTBOOK
            f, df = (1 + s5 * r + LD(5) / 3 * r2) * np.exp(-s5 * r), -LD(5) / 6 * (1 + s5 * r) * np.exp(-s5 * r)
        out += LD(t["c"]) * (2 * df[..., None] * diff * il ** 2 if deriv else f)
    return out


def feats(Omega, phase, amp, Z, deriv=False):
    """Phi(Z) (m, R), or with deriv dPhi/dz (m, R, NDim)."""
    O = Omega.astype(LD)
    arg = Z.astype(LD) @ O.T + phase.astype(LD)
    if not deriv:
        return amp.astype(LD) * np.cos(arg)
    return (-amp.astype(LD) * np.sin(arg))[..., None] * O[None, :, :]
