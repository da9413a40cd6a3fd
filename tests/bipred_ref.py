"""The B-frame rule of include/vcf_amd.h ("B-frames") in numpy, written from
the rule's text: the reference for vcf_ipp_bipred_residual and
vcf_ipp_bipred_reconstruct, the GOP structure of --bframes, and the whole
coding loop over tests/subpel_ref.py and the oracle's 2D-DCT round trip.
Nothing here calls the library."""
import numpy as np

import subpel_ref as R
from oracle import oracle as O

# subpel_sequence(64, 96, 7, seed=SEQ_SEED) with -G 5 -M 16 -S 4: every mode takes >= 5 % of the B blocks at
# --bframes 1 and 2, --subpel 1 and 4 (tests/test_bframes.py checks it on this restatement alone)
SEQ_SEED = 34


def gop_types(L, N):
    """I, anchors at a + N + 1 clamped to the last frame, B strictly between anchors."""
    t = ["B"] * L
    t[0] = "I"
    a = 0
    while a < L - 1:
        a = min(a + N + 1, L - 1)
        t[a] = "P"
    return "".join(t)


def _candidates(cf, cb):
    cf, cb = cf.astype(np.int64), cb.astype(np.int64)
    return np.stack([cf, cb, (cf + cb + 1) >> 1])


def bipred_modes(cur, cf, cb, bs):
    """(H//bs, W//bs) u8: per full block the argmin of (SAD_m, m) over the block's bs*bs*3 bytes."""
    H, W = cur.shape[:2]
    hb, wb = H // bs, W // bs
    d = np.abs(cur.astype(np.int64)[None] - _candidates(cf, cb))[:, :hb * bs, :wb * bs]
    sad = d.reshape(3, hb, bs, wb, bs, 3).sum(axis=(2, 4, 5))
    return np.argmin(sad, axis=0).astype(np.uint8).reshape(hb, wb)   # the first minimum: ties to the lower m


def _pred(cf, cb, modes, bs):
    H, W = cf.shape[:2]
    p = _candidates(cf, cb)
    pred = np.zeros((H, W, 3), np.int64)
    for by in range(H // bs):
        for bx in range(W // bs):
            i, j = by * bs, bx * bs
            pred[i:i + bs, j:j + bs] = p[int(modes[by, bx]), i:i + bs, j:j + bs]
    return pred


def bipred_residual(cur, cf, cb, bs):
    """(modes, clip(cur - pred + 128)) with pred = 0 outside the full-block area."""
    modes = bipred_modes(cur, cf, cb, bs)
    res = np.clip(cur.astype(np.int64) - _pred(cf, cb, modes, bs) + 128, 0, 255).astype(np.uint8)
    return modes, res


def bipred_reconstruct(cf, cb, modes, rec, bs):
    return np.clip(_pred(cf, cb, modes, bs) + rec.astype(np.int64) - 128, 0, 255).astype(np.uint8)


def dct_round_trip(Q):
    def rt(img):
        H, W = img.shape[:2]
        return O.decode_frame(O.encode_frame(img, Q), H, W, Q)
    return rt


def loop(frames, gop, N, bs, sr, fast, Q, subpel, rt=None):
    """The coding loop with B-frames over a spatial round trip rt (default: the oracle's 2D-DCT at Q)
    -> (decoded frames in display order, anchor fields, B fields (n_B, 2, hb, wb, 2), B modes, types)."""
    rt = rt or dct_round_trip(Q)
    recon, mvs, bmv, bmodes, types = {}, [], [], [], ""
    for g0 in range(0, len(frames), gop):
        t = gop_types(min(gop, len(frames) - g0), N)
        types += t
        recon[g0] = rt(frames[g0])
        anchors = [i for i, c in enumerate(t) if c != "B"]
        for a, c in zip(anchors, anchors[1:]):
            ra, cur = recon[g0 + a], frames[g0 + c]
            mv = R.block_matching(ra, cur, bs, sr, fast, subpel)
            comp = R.motion_compensate(ra, mv, bs)
            rc = recon[g0 + c] = O.ipp_reconstruct(comp, rt(O.ipp_residual(cur, comp)))
            mvs.append(mv)
            for d in range(a + 1, c):
                cur = frames[g0 + d]
                mf, mb = R.block_matching(ra, cur, bs, sr, fast, subpel), R.block_matching(rc, cur, bs, sr, fast, subpel)
                cf, cb = R.motion_compensate(ra, mf, bs), R.motion_compensate(rc, mb, bs)
                modes, res = bipred_residual(cur, cf, cb, bs)
                recon[g0 + d] = bipred_reconstruct(cf, cb, modes, rt(res), bs)
                bmv.append(np.stack([mf, mb]))
                bmodes.append(modes)
    hb, wb = frames[0].shape[0] // bs, frames[0].shape[1] // bs
    return ([recon[i] for i in sorted(recon)], mvs, np.array(bmv, np.float32).reshape(len(bmv), 2, hb, wb, 2),
            np.array(bmodes, np.uint8).reshape(len(bmodes), hb, wb), types)
