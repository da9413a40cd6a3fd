"""Container version 4 (-c TCBAAC2D: tiles with a two-dimensional context)
against version 3 (-c TCBAACP) and the serial stream (-c CBAAC).

    python scripts/bench_tcbaac2d.py --rate  [--out profiles/tcbaac2d_rate.json]
    python scripts/bench_tcbaac2d.py --time  [--out profiles/tcbaac2d_bench.json]

--rate (host coders only, no GPU): whole-file bytes -- headers and prior rows
included -- of the DCT indices (B = 8, numpy restatement of the encode) of
the synthetic frames scripts/bench_tcbaac.py codes (synth_frame(H, W, 0),
1080p and 4K), at Q = 8 and Q = 32: version 4 (64 x 64 tiles, nclass 1..8)
over version 3 (CLASS_SEG segments, 8 classes) and over the serial stream
(vcf_cbaac_encode plus its 16-byte header).

--time (GPU): the kernels on device-resident indices of a 1080p frame,
Q = 32 -- prior rows + encode, and decode from a payload in HBM -- per frame
and per batch of 256 frames, version 4 and version 3 in the same process on
the same device (v3_wave: version 3 held to its one-wave-per-segment
kernels, the mapping version 4 has): a settle phase of launches, then HIP events around `reps`
back-to-back launches, the median of `rounds` such groups."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from vcf_amd import tcbaac as T
from vcf_amd.synthetic import synth_frame


def indices(H, W, Q):
    from oracle import ref_numpy
    return np.ascontiguousarray(ref_numpy.encode_frame(synth_frame(H, W, 0), Q))


def rate():
    from vcf_amd.cbaac import encode_symbols
    rows = []
    for H, W in ((1080, 1920), (2160, 3840)):
        for Q in (8, 32):
            k = indices(H, W, Q)
            v3 = len(T.HostTiledCBAACCodec(0, T.CLASS_SEG, True, T.PRIOR_CLASSES).compress(k).getvalue())
            serial = 4 + 4 * k.ndim + len(encode_symbols(k.ravel(), 0))
            for nclass in (1, 2, 4, 8):
                data = T.HostTiledCBAACCodec(nclass=nclass, ctx2d=True).compress(k).getvalue()
                payload = T._parse2d(data)[6]
                rows.append(dict(case="tcbaac2d_rate", frame=[H, W, 3], Q=Q, tile=list(T.TILE_2D), nclass=nclass,
                                 v4_bytes=len(data), v4_header_bytes=len(data) - len(payload), v3_bytes=v3,
                                 serial_bytes=serial, v4_over_v3=round(len(data) / v3, 4),
                                 v4_over_serial=round(len(data) / serial, 4)))
                print(json.dumps(rows[-1]), flush=True)
    return rows


def timed(fn, stream, reps, rounds=5, settle=3):
    from vcf_amd.device import Event
    for _ in range(settle):
        fn()
    stream.synchronize()
    ts = []
    for _ in range(rounds):
        a, b = Event(), Event()
        a.record(stream)
        for _ in range(reps):
            fn()
        b.record(stream)
        b.synchronize()
        ts.append(a.elapsed_ms(b) / reps)
    return float(np.median(ts))


def time_gpu():
    import vcf_amd._lib as L
    from vcf_amd import dct as D
    from vcf_amd.device import DeviceBuffer, set_device
    set_device(0)
    H, W, Q = 1080, 1920, 32
    k = np.ascontiguousarray(D.encode(synth_frame(H, W, 0), Q))
    shape, n = k.shape, k.size
    th, tw = T.TILE_2D
    K = T.PRIOR_CLASSES
    rows = []
    for F, reps in ((1, 20), (256, 2)):
        buf = DeviceBuffer.from_array(np.tile(k.ravel(), F))
        res = {}
        # v3_wave: version 3 held to its one-wave-per-segment kernels (what version 4 has); v3 alone picks
        # one lane per segment from 4608 segments on
        for name, fb in (("v4", T.FrameBatch2D(F, shape, T.TILE_2D, K)),
                         ("v3", T.FrameBatch(F, n, 0, T.CLASS_SEG, prior=True, nclass=K)),
                         ("v3_wave", T.FrameBatch(F, n, 0, T.CLASS_SEG, prior=True, nclass=K, kernel=1))):
            enc_ms = timed(lambda: fb.launch(buf), fb.stream, reps)
            got = fb.download()
            payload = b"".join(e[1] for e in got)
            offs, base = [], 0
            for e in got:
                offs.append(np.concatenate([[0], np.cumsum(e[0])]) + base)
                base += len(e[1])
            src = DeviceBuffer.from_array(np.frombuffer(payload, np.uint8))
            doffs = DeviceBuffer.from_array(np.concatenate(offs).astype(np.int64))
            dpr = DeviceBuffer.from_array(np.ascontiguousarray(np.stack([e[2] for e in got]), np.uint16))
            out = DeviceBuffer(F * n)
            h = fb.stream.handle
            if name == "v4":
                def dec():
                    L.call("vcf_cbaac_tiled2d_decode_frames", src.ptr, doffs.ptr, F, *shape, dpr.ptr, K, th, tw, out.ptr,
                           n, h)
            else:
                def dec():
                    L.call_v(fb.kernel, "vcf_cbaac_tiled_decode_classes", src.ptr, doffs.ptr, F, n, 0, dpr.ptr, K,
                             T.CLASS_SEG, out.ptr, n, h)
            dec_ms = timed(dec, fb.stream, reps)
            ok = bool(np.array_equal(out.download(np.empty(F * n, np.uint8)).reshape(F, *shape)[F - 1], k))
            res[name] = dict(encode_ms=round(enc_ms, 3), decode_ms=round(dec_ms, 3), units=fb.ns,
                             payload_bytes_per_frame=len(payload) // F, round_trip=ok)
        rows.append(dict(case="tcbaac2d_time", frame=[H, W, 3], Q=Q, frames=F, v4=res["v4"], v3=res["v3"],
                         v3_wave=res["v3_wave"],
                         encode_v4_over_v3_wave=round(res["v4"]["encode_ms"] / res["v3_wave"]["encode_ms"], 3),
                         decode_v4_over_v3_wave=round(res["v4"]["decode_ms"] / res["v3_wave"]["decode_ms"], 3),
                         encode_v4_over_v3=round(res["v4"]["encode_ms"] / res["v3"]["encode_ms"], 3),
                         decode_v4_over_v3=round(res["v4"]["decode_ms"] / res["v3"]["decode_ms"], 3)))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rate", action="store_true")
    ap.add_argument("--time", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    rows = (rate() if args.rate else []) + (time_gpu() if args.time else [])
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
