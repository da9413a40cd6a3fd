"""The decoder inputs of tests/decoder_inputs.py, checked on the host: the
inflate corpus is not hollow and zlib's verdict on every entry is the
recorded one; the hand-built streams are valid or invalid as named; the host
CBAAC decoders define an answer for every payload; and the C oracle's DCT
decode, the reference the GPU is held to where its int16 arithmetic wraps,
equals a short numpy restatement of 2D-DCT.py's decode written here.
No GPU is needed, but the built libraries are: the host CBAAC coder lives in
libvcf_amd.so (as for tests/test_tcbaac.py) and the oracle is compiled C.
Run with -s for the corpus counts and the wrapped-sample shares."""
import zlib

import numpy as np
import pytest

import decoder_inputs as DI
from oracle import oracle as O


# ---- inflate ----------------------------------------------------------------------------

def test_inflate_corpus_is_not_hollow():
    corpus, st = DI.inflate_corpus(), DI.reseal_stats()
    accepted = sum(w is not None for _, _, _, w in corpus)
    rejected = len(corpus) - accepted
    print(f"\ninflate corpus: {len(corpus)} strips, accepted {accepted}, rejected {rejected}, resealed "
          f"{st['resealed']} of {st['flips']} flips ({st['differ']} differ from their base, "
          f"{st['length_differs']} in length)")
    assert accepted >= 1000 and rejected >= 1000
    assert st["differ"] >= 0.9 * st["resealed"]
    assert st["length_differs"] >= 100
    assert len({n for n, _, _, _ in corpus}) == len(corpus)       # names are unique
    for name, _, out_len, want in corpus:
        assert want is None or len(want) == out_len, name
    groups = {n.split(":")[0] for n, _, _, _ in corpus}
    assert groups == {"enc", "reseal", "flip", "trunc", "len-1", "len+1", "hand"}
    for g in ("enc", "reseal"):                                    # what an encoder shape or a reseal is: valid
        assert all(w is not None for n, _, _, w in corpus if n.startswith(g + ":")), g


def test_zlib_verdict_is_the_recorded_one():
    for name, stream, out_len, want in DI.inflate_corpus():
        try:
            got = zlib.decompress(stream)
            if len(got) != out_len:
                got = None
        except zlib.error:
            got = None
        assert got == want, name


def test_hand_built_streams():
    status = DI.hand_status()
    hand = [e for e in DI.inflate_corpus() if e[0].startswith("hand:")]
    assert len(hand) == len(status) == 26
    for name, stream, out_len, want in hand:
        if status[name] == 0:
            assert want is not None and zlib.decompress(stream) == want, name
        else:
            assert want is None, name
            with pytest.raises(zlib.error):
                zlib.decompress(stream)
    assert sorted(set(status.values())) == [-4, -3, -2, -1, 0]


# ---- CBAAC --------------------------------------------------------------------------------

def host_encode(seg, order, row):
    """The host coder on one segment (the `encode` of DI.cbaac_payloads)."""
    from vcf_amd import tcbaac as T
    from vcf_amd.cbaac import encode_symbols
    if row is None:
        return encode_symbols(seg, order)
    return T.host_segments_prior(seg, row, 1 << 20, order)[0]


def host_decode(entry):
    """The host decoders, segment by segment, on a payload of DI.cbaac_payloads."""
    from vcf_amd import tcbaac as T
    from vcf_amd.cbaac import decode_symbols
    _, order, seg_len, n, prior, seg_bytes, payload, _ = entry
    offs = np.concatenate([[0], np.cumsum(seg_bytes)])
    out = []
    for s in range(len(seg_bytes)):
        data = payload[offs[s]:offs[s + 1]]
        m = min(seg_len, n - s * seg_len)
        row = DI.segment_row(prior, s, len(seg_bytes))
        out.append(decode_symbols(data, m, order) if row is None else T.host_decode_prior(data, m, row, order))
    return np.concatenate(out)


@pytest.mark.parametrize("order", [0, 1])
@pytest.mark.parametrize("seg_len", [256, 4096])
def test_host_cbaac_decoders_define_every_payload(order, seg_len):
    from vcf_amd import tcbaac as T
    entries = DI.cbaac_payloads(host_encode, order, seg_len)
    assert len(entries) == 5 * 3 * len(DI.PAYLOAD_KINDS)
    assert {e[0] for e in entries} == set(DI.PAYLOAD_KINDS)
    def group(e):                                  # the payloads made from one valid encoding
        return e[3], 0 if e[4] is None else e[4].shape[0] if e[4].ndim == 2 else 1

    valid = {group(e): e[7] for e in entries if e[7] is not None}
    assert len(valid) == 15 and {group(e) for e in entries} == set(valid)
    changed = 0
    for e in entries:
        kind, _, _, n, prior, seg_bytes, payload, sym = e
        if prior is not None:
            T.check_prior(prior)
        assert len(seg_bytes) == (n + seg_len - 1) // seg_len and int(seg_bytes.sum()) == len(payload)
        a, b = host_decode(e), host_decode(e)
        assert a.size == n and a.dtype == np.uint8 and np.array_equal(a, b), (kind, n)
        assert (sym is not None) == (kind == "valid")
        if sym is not None:
            assert np.array_equal(a, sym), (kind, n)
        else:
            changed += not np.array_equal(a, valid[group(e)])
    # most of the other payloads decode to other symbols (n = 1, a fifth of them, may not): they
    # reach coder states the encoder's streams do not
    assert changed >= 0.5 * (len(entries) - 15)


# ---- DCT decode: the oracle against numpy ---------------------------------------------------

def _idct3_matrix(N=8):
    n, k = np.arange(N)[:, None], np.arange(N)[None, :]
    M = np.sqrt(2.0 / N) * np.cos(np.pi * k * (2 * n + 1) / (2 * N))
    M[:, 0] = 1.0 / np.sqrt(N)
    return M


def _wrap16(a):
    return np.asarray(a, np.int64).astype(np.int16)


def decode_numpy(k, H, W, Q, flags=0):
    """2D-DCT.py's decode of 8x8 blocks in numpy -> (u8 H x W x 3, the float64
    inverse transform cropped to H x W, per-sample mask of int16 wraps)."""
    Hp, Wp = k.shape[:2]
    v32 = Q * (k.astype(np.int16) - 128).astype(np.int32)
    v = _wrap16(v32)                                               # Q * k in int16
    wq = v32 != v
    if not flags & 1:                                              # subbands -> blocks
        v, wq = (a.reshape(8, Hp // 8, 8, Wp // 8, 3).transpose(1, 0, 3, 2, 4).reshape(Hp, Wp, 3) for a in (v, wq))
    M = _idct3_matrix()
    f = np.einsum("ny,mx,aybxc->anbmc", M, M, v.reshape(Hp // 8, 8, Wp // 8, 8, 3).astype(np.float64))
    f = f.reshape(Hp, Wp, 3)
    wq = np.broadcast_to(wq.reshape(Hp // 8, 8, Wp // 8, 8, 3).any(axis=(1, 3, 4))[:, None, :, None],
                         (Hp // 8, 8, Wp // 8, 8)).reshape(Hp, Wp)
    t, l = (Hp - H) // 2, (Wp - W) // 2
    f, wq = f[t:t + H, l:l + W], wq[t:t + H, l:l + W]
    ct = np.trunc(f).astype(np.int64)
    wi = (ct != _wrap16(ct)).any(axis=2)
    Y, Co, Cg = (_wrap16(ct[..., c]).astype(np.int64) for c in range(3))
    wc = np.zeros((H, W, 3), bool)
    outs = []
    for c, (s1, s2) in enumerate(((1, -1), (0, 1), (-1, -1))):     # r = (Y + Co) - Cg, g = Y + Cg, b = (Y - Co) - Cg
        a = Y + s1 * Co
        a16 = _wrap16(a).astype(np.int64)
        b = a16 + s2 * Cg
        b16 = _wrap16(b).astype(np.int64)
        o = b16 + 128
        wc[..., c] = (a != a16) | (b != b16) | (o != _wrap16(o))
        outs.append(np.clip(_wrap16(o), 0, 255).astype(np.uint8))
    return np.stack(outs, axis=2), f, wc | wi[..., None] | wq[..., None]


@pytest.mark.parametrize("shape", [(8, 8), (24, 40)])
def test_oracle_dct_decode_equals_numpy_restatement(shape):
    H, W = shape
    compared = total = 0
    for Q in (1, 32, 64, 255, 30001):
        wrapped = samples = 0
        for flags in (0, 1):
            frames = DI.dct_index_frames(H, W, 1000 + Q + flags)
            for cls, k in zip(DI.PLANE_CLASSES, frames):
                got, f, wrap = decode_numpy(k, H, W, Q, flags)
                want = O.decode_frame(k, H, W, Q, flags)
                safe = (np.abs(f - np.rint(f)) > 1e-6).all(axis=2)   # truncation cannot depend on the rounding order
                assert np.array_equal(got[safe], want[safe]), (cls, Q, flags)
                compared += 3 * int(safe.sum())
                total += 3 * H * W
                wrapped += int(wrap.sum())
                samples += wrap.size
        print(f"\nDCT {H}x{W} Q={Q}: wrapped samples {wrapped / samples:.4f}")
        assert Q < 64 or wrapped > 0
    assert compared >= 0.95 * total, (compared, total)
