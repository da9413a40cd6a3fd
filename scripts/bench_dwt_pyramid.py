"""The 2D-DWT codec's batch path (the pyramid coded in HBM: encode_fns /
decode_fns) against the per-subband host path it replaces, same box, same run.

    python scripts/bench_dwt_pyramid.py [--frames 16] [--reps 3] [--out profiles/dwt_pyramid_bench.json]

16 synthetic 1080p frames (vcf_amd.synthetic.synth_frame), -w bior4.4 -l 5
-q 32, encode and decode, -c TIFF and -c TCBAAC2D:
  batch        encode_fns / decode_fns of this tree;
  per_subband  what the parent commit ran: one transform launch per group, every
               subband downloaded, 3 L + 1 compress calls per frame on 8 host
               threads (its encode_fns), decode_fn frame by frame (its decode_fns).
Each is warmed once and timed `reps` times with the host clock around the whole
call (it ends with the files on disk, all device work waited for); the median
and the spread are reported.  The split of the batch encode (transform, coder,
D2H, file I/O) comes from a separate instrumented pass that waits for the
stream between stages, so its parts do not overlap and do not add up to the
pipelined total.  bytes_per_frame: the 16 subband files of a frame, summed,
mean over the frames, for TIFF, TCBAAC2D and CBAAC (CBAAC over 2 frames: the
serial host coder).  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from vcf_amd import dwt as DW
from vcf_amd.codec import parser as P
from vcf_amd.codec.dwt2d import CoDec
from vcf_amd.codec.eic import write_image
from vcf_amd.synthetic import synth_frame

H, W, LEVELS, WAVELET, Q = 1080, 1920, 5, "bior4.4", 32


def codec(sub, c):
    return CoDec(P.parse(P.dwt_parser(), [sub, "-c", c, "-w", WAVELET, "-l", str(LEVELS), "-q", str(Q)]))


def per_subband_encode(c, pairs):
    """The parent commit's encode_fns: the group's transform, then write_decom_fn per frame on 8 threads."""
    with ThreadPoolExecutor(max_workers=8) as pool:
        imgs = list(pool.map(lambda p: c.encode_read_fn(p[0]), pairs))
        sbs = DW.encode(np.stack(imgs), c.wavelet, c.levels, c.QSS)
        return list(pool.map(lambda i: c.write_decom_fn(sbs[i], pairs[i][1]), range(len(pairs))))


def per_subband_decode(c, pairs):
    return [c.decode_fn(i, o) for i, o in pairs]


def timed(fn, reps):
    fn()                                    # warm-up: code objects, scratch buffers, the page cache
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return dict(median_s=round(statistics.median(ts), 4), min_s=round(min(ts), 4), max_s=round(max(ts), 4), reps=reps)


def split(c, srcs, tmp):
    """The batch encode stage by stage, the stream waited for between stages."""
    st, scratch = c._device()
    imgs = [c.encode_read_fn(s) for s in srcs]
    n = len(imgs)
    planes = DW.subband_planes(H, W, LEVELS)
    _, pb, wb = DW.layout(H, W, LEVELS)
    res = {}
    for rep in range(2):                    # the second pass is the one reported
        din, packed, ws = scratch.get("rgb", n * H * W * 3), scratch.get("packed", n * pb), scratch.get("ws", n * wb)
        t0 = time.perf_counter()
        din.upload(np.stack(imgs), st)
        st.synchronize()
        t1 = time.perf_counter()
        DW.encode_device(din, n, H, W, DW.wavelet_index(WAVELET), LEVELS, Q, packed, ws, st)
        st.synchronize()
        t2 = time.perf_counter()
        coder = c._tiles2d()
        if coder is not None:
            coder.launch(packed, [(f * pb + off, h, w, cc) for f in range(n) for _, off, h, w, cc in planes])
            st.synchronize()
            t3 = time.perf_counter()
            files = coder.streams([(h, w, cc) for _ in range(n) for _, _, h, w, cc in planes])
            t4 = time.perf_counter()
            out = [[(planes[s][0], files[f * len(planes) + s]) for s in range(len(planes))] for f in range(n)]
            res = dict(h2d_ms=(t1 - t0) * 1e3, transform_ms=(t2 - t1) * 1e3, coder_ms=(t3 - t2) * 1e3,
                       d2h_and_headers_ms=(t4 - t3) * 1e3, code_stream_bytes=sum(len(x) for x in files),
                       prior_rows_d2h_bytes=int(n * len(planes) * coder.nclass * 16 * 512))
        else:
            out = c._encode_group(imgs, (H, W, 3))      # transform again + gather + deflate + D2H, not separable here
            t4 = time.perf_counter()
            res = dict(h2d_ms=(t1 - t0) * 1e3, transform_ms=(t2 - t1) * 1e3,
                       group_h2d_transform_coder_d2h_ms=(t4 - t2) * 1e3)
        t5 = time.perf_counter()
        for f in range(n):
            for name, payload in out[f]:
                with open(os.path.join(tmp, f"split{f}_{name}"), "wb") as fh:
                    fh.write(payload if isinstance(payload, bytes) else payload.tobytes())
        res["file_io_ms"] = (time.perf_counter() - t5) * 1e3
    return {k: round(v, 3) if isinstance(v, float) else v for k, v in res.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="profiles/dwt_pyramid_bench.json")
    a = ap.parse_args()
    from vcf_amd.device import device_count
    if device_count() < 1:
        sys.exit("bench_dwt_pyramid: no GPU")
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        srcs = []
        for i in range(a.frames):
            srcs.append(os.path.join(tmp, f"in{i:02d}.png"))
            write_image(srcs[-1], synth_frame(H, W, i))
        names = DW.subband_names(LEVELS)
        bytes_per_frame = {}
        for c_name in ("TIFF", "TCBAAC2D"):
            enc, dec = codec("encode", c_name), codec("decode", c_name)
            ext = enc.file_extension
            e_b = [(s, os.path.join(tmp, f"{c_name}_b{i}")) for i, s in enumerate(srcs)]
            e_p = [(s, os.path.join(tmp, f"{c_name}_p{i}")) for i, s in enumerate(srcs)]
            d_b = [(o, os.path.join(tmp, f"{c_name}_db{i}.png")) for i, (_, o) in enumerate(e_b)]
            d_p = [(o, os.path.join(tmp, f"{c_name}_dp{i}.png")) for i, (_, o) in enumerate(e_p)]
            row = dict(case="dwt_pyramid", codec=c_name, frames=a.frames, frame=[H, W, 3], wavelet=WAVELET,
                       levels=LEVELS, Q=Q,
                       encode_batch=timed(lambda: enc.encode_fns(e_b, batch=a.frames), a.reps),
                       encode_per_subband=timed(lambda: per_subband_encode(enc, e_p), a.reps),
                       decode_batch=timed(lambda: dec.decode_fns(d_b, batch=a.frames), a.reps),
                       decode_per_subband=timed(lambda: per_subband_decode(dec, d_p), a.reps))
            same = all(open(f"{b[1]}_{n}{ext}", "rb").read() == open(f"{p[1]}_{n}{ext}", "rb").read()
                       for b, p in zip(e_b, e_p) for n in names)
            row["files_equal"] = bool(same)
            row["encode_speedup"] = round(row["encode_per_subband"]["median_s"] / row["encode_batch"]["median_s"], 3)
            row["decode_speedup"] = round(row["decode_per_subband"]["median_s"] / row["decode_batch"]["median_s"], 3)
            row["encode_split"] = split(enc, srcs, tmp)
            bytes_per_frame[c_name] = sum(os.path.getsize(f"{b[1]}_{n}{ext}") for b in e_b for n in names) / a.frames
            rows.append(row)
            print(json.dumps(row), flush=True)
        cb = codec("encode", "CBAAC")
        sizes = per_subband_encode(cb, [(s, os.path.join(tmp, f"cbaac{i}")) for i, s in enumerate(srcs[:2])])
        bytes_per_frame["CBAAC"] = sum(sizes) / len(sizes)
    result = dict(script="scripts/bench_dwt_pyramid.py", rows=rows,
                  bytes_per_frame={k: round(v, 1) for k, v in bytes_per_frame.items()},
                  raw_bytes_per_frame=H * W * 3, device="AMD Instinct MI355X (gfx950), one GPU")
    print(json.dumps(result["bytes_per_frame"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
