"""-f deblock on the host: the rule of include/vcf_amd.h (vcf_deblock_u8) as tests/deblock_ref.py
restates it, the parser's surface, the codecs' refusals and the documented default strengths.
Nothing here needs a GPU."""
import numpy as np
import pytest

import deblock_ref as R


def _row(vals):
    """One row of grey pixels as a 1 x n x 3 frame."""
    return np.repeat(np.array(vals, np.uint8)[None, :, None], 3, axis=2)


def test_hand_check():
    """beta = 16, tc = 4: 10 10 10 | 18 18 18 -> 10 11 13 | 15 16 18."""
    out = R.deblock_ref(_row([10, 10, 10, 18, 18, 18]), 4, 0, 1, 16, 4)      # the edge at x = 3
    assert out[0, :, 0].tolist() == [10, 11, 13, 15, 16, 18]
    assert np.array_equal(out[..., 0], out[..., 1]) and np.array_equal(out[..., 0], out[..., 2])
    # the same line down a column
    col = np.ascontiguousarray(np.swapaxes(_row([10, 10, 10, 18, 18, 18]), 0, 1))
    assert R.deblock_ref(col, 4, 1, 0, 16, 4)[:, 0, 0].tolist() == [10, 11, 13, 15, 16, 18]


def test_tc_zero_and_constant_images_are_unchanged():
    img = R.blocky_frames(5, 2, 37, 45, 8, 1, 2)
    assert np.array_equal(R.deblock_ref(img, 8, 1, 2, 64, 0), img)
    flat = np.full((20, 24, 3), 77, np.uint8)
    assert np.array_equal(R.deblock_ref(flat, 4, 0, 0, 4096, 255), flat)


@pytest.mark.parametrize("B,top,left", [(4, 0, 0), (8, 3, 5), (16, 0, 9)])
def test_only_the_two_samples_beside_an_edge_change(B, top, left):
    """p2, q2 and everything further than two samples from an edge keep their values."""
    H, W = 41, 53
    img = R.blocky_frames(6, 1, H, W, B, top, left)[0]
    out = R.deblock_ref(img, B, top, left, 4096, 255)
    assert not np.array_equal(out, img)
    near_x = np.zeros(W, bool)
    for x in R.edges(W, left, B):
        near_x[max(x - 2, 0):x + 2] = True
    near_y = np.zeros(H, bool)
    for y in R.edges(H, top, B):
        near_y[max(y - 2, 0):y + 2] = True
    far = ~near_y[:, None] & ~near_x[None, :]
    assert np.array_equal(out[far], img[far])
    v = R.pass_v(img, B, left, 4096, 255)[0]
    assert np.array_equal(v[:, ~near_x], img[:, ~near_x])
    assert np.array_equal(out[~near_y], v[~near_y])


def test_lines_near_a_border_are_left_alone():
    """An edge at x = 1, 2, W - 2 or W - 1 has no p2 or q2 inside the frame: its lines stay."""
    W = 24
    img = R.blocky_frames(7, 1, 6, W, 8, 0, 0, amp=0)[0]
    for x in (1, 2, W - 2, W - 1):
        left = (-x) % 8
        assert x in R.edges(W, left, 8)
        frame = img.copy()
        frame[:, :x] = 100
        frame[:, x:] = 108               # a step every interior edge would smooth
        out, mv = R.pass_v(frame, 8, left, 4096, 255)
        assert mv["on"].shape[1] == len(R.edges(W, left, 8)) - 1
        lo, hi = max(x - 2, 0), min(x + 2, W)
        assert np.array_equal(out[:, lo:hi], frame[:, lo:hi])
    # x = 3 and x = W - 3 are filtered
    for x in (3, W - 3):
        frame = np.full((2, W, 3), 100, np.uint8)
        frame[:, x:] = 108
        assert not np.array_equal(R.pass_v(frame, 8, (-x) % 8, 4096, 255)[0], frame)


def test_pass_order_is_v_then_h():
    img = R.blocky_frames(8, 1, 24, 24, 8, 0, 0)[0]
    out = R.deblock_ref(img, 8, 0, 0, 64, 8)
    v_then_h = R.pass_h(R.pass_v(img, 8, 0, 64, 8)[0], 8, 0, 64, 8)[0]
    h_then_v = R.pass_v(R.pass_h(img, 8, 0, 64, 8)[0], 8, 0, 64, 8)[0]
    assert np.array_equal(out, v_then_h)
    assert not np.array_equal(out, h_then_v)


def test_gpu_inputs_reach_every_branch():
    """The inputs of tests/test_deblock_gpu.py, through the restatement: every branch of the rule is
    taken at least once, so the bit-equality there says something about each of them."""
    count = dict.fromkeys(R.MASKS, 0)
    v_changed_read_by_h = 0
    for case in R.GPU_CASES:
        H, W, B, top, left = case
        rows = np.zeros(H, bool)
        for y in R.edges(H, top, B):
            if y - 3 >= 0 and y + 2 <= H - 1:
                rows[y - 3:y + 3] = True
        for frame in R.case_frames(case):
            for beta, tc in R.GPU_STRENGTHS:
                _, v, mv, mh = R.deblock_masks(frame, B, top, left, beta, tc)
                for k in R.MASKS:
                    count[k] += int(mv[k].sum()) + int(mh[k].sum())
                v_changed_read_by_h += int((v != frame)[rows].sum())
    print(count, v_changed_read_by_h)
    for k in R.MASKS:
        assert count[k] > 0, k
    assert v_changed_read_by_h > 0


# ---- the command line and the codecs ------------------------------------------------
def _parsers():
    from vcf_amd.codec import parser as P
    return {"2D-DCT": P.dct_parser, "2D-KLT": P.klt_parser, "2D-LBT": P.lbt_parser}


def test_default_strength_is_the_documented_rule():
    """DESIGN.md §4.19 and --help: beta = Q, tc = max(1, Q // 8)."""
    from vcf_amd import deblock as DB
    from vcf_amd.codec import parser as P
    for Q in (1, 4, 7, 8, 9, 16, 32, 33, 64, 128, 1000):
        assert DB.default_strength(Q) == (Q, max(1, Q // 8))
    assert DB.strength(32) == (32, 4) and DB.strength(32, 10, None) == (10, 4) and DB.strength(32, None, 0) == (32, 0)
    text = P.dct_parser(filter="deblock").parse_known_args  # noqa: F841  (the parser builds)
    import contextlib
    import io
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit):
        P.dct_parser(filter="deblock").parse_args(["decode", "--help"])
    help_text = " ".join(buf.getvalue().split())
    assert "beta = Q" in help_text and "max(1, Q // 8)" in help_text
    assert DB.crop_offsets(61, 77, 8) == (1, 1) and DB.crop_offsets(64, 64, 8) == (0, 0) == R.crop_offsets(64, 64, 8)
    assert DB.crop_offsets(13, 29, 4) == R.crop_offsets(13, 29, 4) == (1, 1)


def test_flags_join_the_parser_only_with_f_deblock():
    from vcf_amd.codec import parser as P
    assert P.filter_of(["decode", "-f", "deblock"]) == "deblock"
    assert P.filter_of(["decode"]) == "no_filter" and P.filter_of(["decode", "--filter", "NLM"]) == "NLM"
    for name, make in _parsers().items():
        plain = P.parse(make(), ["decode"])
        assert not hasattr(plain, "deblock_beta") and not hasattr(plain, "deblock_tc"), name
        assert vars(P.parse(make(filter="no_filter"), ["decode"])) == vars(plain)
        ns = P.parse(make(filter="deblock"), ["decode", "-f", "deblock", "--deblock_beta", "20", "--deblock_tc", "3"])
        assert (ns.filter, ns.deblock_beta, ns.deblock_tc) == ("deblock", 20, 3), name
        ns = P.parse(make(filter="deblock"), ["decode", "-f", "deblock"])
        assert ns.deblock_beta is None and ns.deblock_tc is None
        without = {k: v for k, v in vars(ns).items() if not k.startswith("deblock_")}
        assert without == {**vars(plain), "filter": "deblock"}
        enc = P.parse(make(filter="deblock"), ["encode"])          # decode-only flags
        assert vars(enc) == vars(P.parse(make(), ["encode"]))
    for t in ("2D-DCT", "2D-KLT", "2D-LBT"):
        plain = P.parse(P.iii_parser(transform=t), ["decode", "-T", t])
        assert not hasattr(plain, "deblock_beta")
        ns = P.parse(P.iii_parser(transform=t, filter="deblock"), ["decode", "-T", t, "-f", "deblock", "--deblock_tc", "2"])
        assert (ns.filter, ns.deblock_beta, ns.deblock_tc) == ("deblock", None, 2)
    assert not hasattr(P.rd_curve_parser().parse_args([]), "filter")
    ns = P.rd_curve_parser(filter="deblock").parse_args(["-f", "deblock", "--deblock_beta", "9"])
    assert (ns.filter, ns.deblock_beta, ns.deblock_tc) == ("deblock", 9, None)


def test_block_codecs_accept_f_deblock_when_decoding():
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.dct2d import CoDec as DCT
    from vcf_amd.codec.klt2d import CoDec as KLT
    from vcf_amd.codec.lbt2d import CoDec as LBT
    for make, C, extra in ((P.dct_parser, DCT, []), (P.dct_parser, DCT, ["-B", "4"]), (P.dct_parser, DCT, ["-B", "16", "-x"]),
                           (P.dct_parser, DCT, ["-p"]), (P.klt_parser, KLT, []), (P.lbt_parser, LBT, ["-B", "4"])):
        c = C(P.parse(make(filter="deblock"), ["decode", "-f", "deblock"] + extra))
        assert c.deblock == (None, None)
        c = C(P.parse(make(filter="deblock"), ["decode", "-f", "deblock", "--deblock_beta", "5", "--deblock_tc", "1"] + extra))
        assert c.deblock == (5, 1)
        assert C(P.parse(make(), ["decode"] + extra)).deblock is None
    c = DCT(P.parse(P.dct_parser(quantizer="LloydMax", filter="deblock"), ["decode", "-a", "LloydMax", "-f", "deblock"]))
    assert c.deblock == (None, None)
    with pytest.raises(ValueError):
        DCT(P.parse(P.dct_parser(filter="deblock"), ["decode", "-f", "deblock", "--deblock_tc", "-1"]))


def test_f_deblock_is_refused_where_it_cannot_run():
    from vcf_amd.codec import parser as P
    from vcf_amd.codec.dct2d import CoDec as DCT
    from vcf_amd.codec.dwt2d import CoDec as DWT
    from vcf_amd.codec.iii import transform_codec
    from vcf_amd.codec.ipp import codec_class
    from vcf_amd.codec.klt2d import CoDec as KLT
    from vcf_amd.codec.lbt2d import CoDec as LBT
    from vcf_amd.codec.mdct2d import CoDec as MDCT
    from vcf_amd.codec import pixel, vq
    fd = ["decode", "-f", "deblock"]
    refused = [(DCT, P.parse(P.dct_parser(filter="deblock"), fd + ["-B", "2"]), "-B 2"),
               (DCT, P.parse(P.dct_parser(filter="deblock"), fd + ["-B", "3"]), "-B 3"),
               (KLT, P.parse(P.klt_parser(filter="deblock"), fd + ["-B", "2"]), "-B 2"),
               (LBT, P.parse(P.lbt_parser(filter="deblock"), fd + ["-B", "3"]), "-B 3"),
               (MDCT, P.parse(P.mdct_parser(), fd), "lapped"),
               (DWT, P.parse(P.dwt_parser(), fd), "2D-DWT"),
               (transform_codec, P.parse(P.iii_parser(transform="2D-MDCT", filter="deblock"), fd + ["-T", "2D-MDCT"]), "lapped"),
               (transform_codec, P.parse(P.iii_parser(transform="2D-DWT", filter="deblock"), fd + ["-T", "2D-DWT"]), "2D-DWT"),
               (codec_class("2D-DCT"), P.parse(P.ipp_parser(), fd), "prediction loop"),
               (vq.VQCoDec if hasattr(vq, "VQCoDec") else None, P.parse(P.build_vq_parser(), fd), "no block grid"),
               (vq.ColorVQCoDec if hasattr(vq, "ColorVQCoDec") else None, P.parse(P.build_color_vq_parser(), fd), "no block grid")]
    for name in ("DeadzoneCoDec", "YCoCgCoDec", "YCrCbCoDec", "LloydMaxCoDec"):
        if hasattr(pixel, name):
            parser = {"DeadzoneCoDec": P.deadzone_parser, "YCoCgCoDec": P.ycocg_parser, "YCrCbCoDec": P.ycrcb_parser,
                      "LloydMaxCoDec": P.lloydmax_parser}[name]
            refused.append((getattr(pixel, name), P.parse(parser(), fd), "no block grid"))
    assert all(c is not None for c, _, _ in refused)
    for C, ns, reason in refused:
        with pytest.raises(NotImplementedError, match=reason):
            C(ns)
    # the reference's own filters stay refused everywhere
    for name in ("gaussian_blur", "NLM", "BM3D"):
        for C, make in ((DCT, P.dct_parser), (KLT, P.klt_parser), (LBT, P.lbt_parser), (MDCT, P.mdct_parser),
                        (DWT, P.dwt_parser)):
            with pytest.raises(NotImplementedError):
                C(P.parse(make(), ["decode", "-f", name]))
    from vcf_amd.codec.rde import rd_curve
    with pytest.raises(NotImplementedError):
        rd_curve(np.zeros((16, 16, 3), np.uint8), [32], filter="gaussian_blur")
