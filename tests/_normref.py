"""Extended-precision reference of the Gauss-Newton diagonal blocks (BAProblem.normal_equations), from a given
per-observation residual and Jacobian: U_c = sum Jc^T Jc, gc = sum Jc^T r per camera, V_p = sum Jp^T Jp, gp = sum Jp^T r
per point, summed in np.longdouble.  Alongside, the sums of absolute products S_ab = sum |J_a J_b| (and sum |J_a r|)
that bound the rounding of ANY f64 summation order: |dev - ref| <= (k + 4) * 2^-53 * S_ab for a block of k
observations (each product rounds once, the two rows' products add once, k - 1 additions follow)."""
import numpy as np

LD = np.longdouble
U53 = 2.0 ** -53


def blocks(r, Jc, Jp, cam_of, pt_idx, n_cam, n_pts):
    """r [n,2], Jc [n,2,9], Jp [n,2,3] (f64, any layout reshaping to those), cam_of / pt_idx [n] -> dict of
    U [n_cam,9,9], gc [n_cam,9], V [n_pts,3,3], gp [n_pts,3] (longdouble), their S bounds (SU, Sgc, SV, Sgp), the
    observation counts kc [n_cam], kp [n_pts] and sum_sq = sum |r|^2."""
    n = len(cam_of)
    r = np.asarray(r, dtype=np.float64).reshape(n, 2).astype(LD)
    Jc = np.asarray(Jc, dtype=np.float64).reshape(n, 2, 9).astype(LD)
    Jp = np.asarray(Jp, dtype=np.float64).reshape(n, 2, 3).astype(LD)
    cam_of = np.asarray(cam_of, dtype=np.int64)
    pt_idx = np.asarray(pt_idx, dtype=np.int64)
    out = {}
    for key, J, idx, m, w in (("U", Jc, cam_of, n_cam, 9), ("V", Jp, pt_idx, n_pts, 3)):
        g = "gc" if key == "U" else "gp"
        JJ = np.einsum("nia,nib->nab", J, J)                       # per-observation Jc^T Jc, rows summed
        AJJ = np.einsum("nia,nib->nab", np.abs(J), np.abs(J))
        Jr = np.einsum("nia,ni->na", J, r)
        AJr = np.einsum("nia,ni->na", np.abs(J), np.abs(r))
        B = np.zeros((m, w, w), dtype=LD)
        SB = np.zeros((m, w, w), dtype=LD)
        G = np.zeros((m, w), dtype=LD)
        SG = np.zeros((m, w), dtype=LD)
        np.add.at(B, idx, JJ)
        np.add.at(SB, idx, AJJ)
        np.add.at(G, idx, Jr)
        np.add.at(SG, idx, AJr)
        out[key], out["S" + key], out[g], out["S" + g] = B, SB, G, SG
    out["kc"] = np.bincount(cam_of, minlength=n_cam)
    out["kp"] = np.bincount(pt_idx, minlength=n_pts)
    out["sum_sq"] = np.sum(r * r)
    return out


def bound(S, k):
    """the per-entry bound (k + 4) 2^-53 S for blocks with k observations (k broadcast over the block's entries)"""
    k = np.asarray(k, dtype=np.float64).reshape((-1,) + (1,) * (np.ndim(S) - 1))
    return (k + 4.0) * U53 * np.asarray(S, dtype=np.float64)


def excess(dev, ref, S, k):
    """largest |dev - ref| / bound (<= 1 passes; 0/0 entries count 0)"""
    err = np.abs(np.asarray(dev, dtype=LD) - ref).astype(np.float64)
    b = bound(S, k)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0.0, 0.0, err / b)
    return float(np.max(q)) if q.size else 0.0


def check(dev, ref, kind):
    """assert dev = (U, gc, V, gp) lies within the bound of ref = blocks(...) entry by entry"""
    U, gc, V, gp = (np.asarray(a, dtype=np.float64) for a in dev)
    for name, a, key, S, k in (("U", U, "U", "SU", "kc"), ("gc", gc, "gc", "Sgc", "kc"), ("V", V, "V", "SV", "kp"),
                               ("gp", gp, "gp", "Sgp", "kp")):
        x = excess(a, ref[key], ref[S], ref[k])
        assert x <= 1.0, "%s %s: error %.3g x the bound" % (kind, name, x)
