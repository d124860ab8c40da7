"""4:2:2 and 4:4:4 chroma on the GPU: the new instantiations of the two clip
kernels against the fp64 oracle, jpeg_idct and jpeg_huff (interval and
subsequence forms) on 4:2:2 / 4:4:4 records against the host decoders, the
decoders end to end against PIL and the oracle, one loader call per container,
and the op with one crop box against a raw launch with that box. Inputs, damage
tables and bounds are tests/test_chroma_cpu.py's."""
import ctypes
import os

import numpy as np
import pytest
import torch

import decode_oracle as orc
import decode_oracle_chroma as occ
from rnb_amd.models.r2p1d.decoder import MjpegDecoder, Y4mDecoder
from rnb_amd.ops import video as vops
from rnb_amd.utils import mjpeg, y4m
from test_chroma_cpu import (GOLDEN_CHROMA, SAMPLINGS, SUBSEQ, WRITTEN, build_written,
                             check_clip_case, check_pil_rgb, chroma_frames, damaged_records,
                             stream_case, y4m_planes)
from test_mjpeg_cpu import check_band

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CPU = torch.device("cpu")
# test_gpu_mjpeg.py's bound for a GPU decoder against the CPU-device one: the IDCT
# kernel and its mirror may round a tie differently by one level
MIRROR_TOL = 0.051


@pytest.fixture(scope="module")
def written(tmp_path_factory):
    return build_written(tmp_path_factory.mktemp("chroma_gpu"))


# -- clip kernels ------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c[0] for c in occ.cases("422")])
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_clip_kernels_against_oracle(sampling, name):
    """Offsets in the kernel arguments: {BT.601, JFIF} x {422, 444} of both
    kernels, fp32 within the oracle's tolerance and bf16 = RNE(fp32) bit for
    bit; ``bt601_aa_wide`` is wider than one column tile of the antialias kernel."""
    check_clip_case(sampling, name, DEV, surface=name == "jfif_bil_45x33")


@pytest.mark.parametrize("name", ["bt601_bil_up", "jfif_bil_45x33", "bt601_aa_full", "jfif_aa_up"])
@pytest.mark.parametrize("sampling", SAMPLINGS)
def test_clip_kernels_65_clips_use_the_device_tables(sampling, name):
    """65 clips, one more than the 64 rows that fit the kernel arguments: offsets
    and boxes come from the device tables."""
    check_clip_case(sampling, name, DEV, clips=65)


@pytest.mark.parametrize("filt", ["bilinear", "antialias"])
@pytest.mark.parametrize("matrix", ["bt601", "jfif"])
def test_420_entry_points_equal_the_generalised_one(matrix, filt):
    """The op with one crop box and a raw rnb_yuv_to_clip_boxes call with that
    box at sampling 0: bit-equal clips."""
    from rnb_amd.ops.native import kernels
    y, u, v = orc.noise_planes(46, 34, 2, 77, matrix)
    buf, stride, pl = orc.pack_i420(y, u, v, 7)
    t = torch.from_numpy(buf).to(DEV)
    crop = (3.5, 1.25, 40.0, 30.0)
    for dtype in (torch.float32, torch.bfloat16):
        old = vops.yuv420_to_clip(t, [0], 2, 46, 34, stride, pl, 16, 12, crop=crop, dtype=dtype,
                                  matrix=matrix, filter=filt)
        new = torch.full_like(old, 3.0)
        offs = (ctypes.c_longlong * 1)(0)
        po = (ctypes.c_longlong * 3)(*pl[:3])
        ps = (ctypes.c_int * 3)(*pl[3:6])
        rc = kernels().lib.rnb_yuv_to_clip_boxes(
            t.data_ptr(), t.numel(), offs, None, 1, 2, 46, 34, stride, po, ps, pl.c_step,
            new.data_ptr(), 16, 12, (ctypes.c_float * 4)(*crop), None,
            (ctypes.c_float * 3)(*vops.KINETICS_MEAN), (ctypes.c_float * 3)(*vops.KINETICS_STD),
            int(dtype == torch.bfloat16), int(matrix == "jfif"), int(filt == "antialias"), 0,
            torch.cuda.current_stream(DEV).cuda_stream)
        torch.cuda.synchronize()
        assert rc == 0 and torch.equal(old, new)


def test_clip_launcher_refusals():
    y, u, v = occ.noise_planes(46, 33, 1, 5, "bt601", "422")
    buf, stride, pl = occ.pack_planar(y, u, v)
    t = torch.from_numpy(buf).to(DEV)
    out = torch.full((1, 1, 4, 4, 4), 9.0, device=DEV)
    with pytest.raises(RuntimeError):                      # a 4:4:4 chroma span in a 4:2:2 frame
        vops.yuv420_to_clip(t, [0], 1, 46, 33, stride, pl, 4, 4, out=out, sampling="444")
    with pytest.raises(RuntimeError):                      # BT.601 4:2:2: odd width
        vops.yuv420_to_clip(t, [0], 1, 45, 33, stride, pl, 4, 4, out=out, sampling="422")
    torch.cuda.synchronize()
    assert torch.all(out == 9.0)                           # nothing was launched


# -- jpeg_idct -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["w422_r3", "w444_r2", "w444_7x9", "w422_7x9",
                                  "noise_q90_422_rows", "noise_q95_444_blocks"])
def test_idct_kernel_against_mirror_and_fp64(written, name):
    idx, want, _, _ = stream_case(written, name)
    fbytes = vops.jpeg_frame_bytes(idx.mw, idx.mh, idx.sampling)[1]
    rec = torch.from_numpy(want)
    mirror = vops.jpeg_idct(rec, 2, idx.mw, idx.mh, sampling=idx.sampling).numpy()
    surf = torch.full((2 * fbytes + 64,), 0xAA, dtype=torch.uint8, device=DEV)
    got = vops.jpeg_idct(rec.to(DEV), 2, idx.mw, idx.mh, out=surf, sampling=idx.sampling)
    assert got.data_ptr() == surf.data_ptr() and got.shape == (2 * fbytes,)
    g = got.cpu().numpy()
    assert torch.all(surf[2 * fbytes:] == 0xAA)            # nothing past the frames
    assert np.abs(g.astype(int) - mirror.astype(int)).max() <= 1     # a tie rounded the other way
    for i in range(2):
        coefs, qt = mjpeg.unpack_record(want[i * idx.record_bytes:(i + 1) * idx.record_bytes],
                                        idx.mw, idx.mh, idx.sampling)
        check_band(g[i * fbytes:(i + 1) * fbytes],
                   mjpeg.idct_planes_f64(coefs, qt, idx.mw, idx.mh, idx.sampling),
                   "%s frame %d" % (name, i))
    # the launcher's checks use this sampling's sizes
    with pytest.raises(RuntimeError, match="contract"):
        vops.jpeg_idct(rec.to(DEV), 2, idx.mw, idx.mh, out=surf[:2 * fbytes - 8],
                       sampling=idx.sampling)
    with pytest.raises(RuntimeError, match="contract"):
        vops.jpeg_idct(rec.to(DEV)[:2 * idx.record_bytes - 16], 2, idx.mw, idx.mh,
                       sampling=idx.sampling)


# -- jpeg_huff -------------------------------------------------------------------------------------
def huff_gpu(scans, offs, n, idx, S):
    rb = idx.record_bytes
    out = torch.full((n * rb + 16,), 0x5A, dtype=torch.uint8, device=DEV)
    rec, status = vops.jpeg_huff(torch.from_numpy(scans).to(DEV), offs, n, idx.mw, idx.mh, out=out,
                                 subseq_bytes=S, sampling=idx.sampling)
    torch.cuda.synchronize()
    assert torch.all(out[n * rb:] == 0x5A)
    return rec.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("name", sorted(WRITTEN) + sorted(GOLDEN_CHROMA))
def test_huff_kernels_equal_the_host_decoder(written, name):
    idx, want, scans, offs = stream_case(written, name)
    for S in (0,) + SUBSEQ:
        rec, status = huff_gpu(scans, offs, 2, idx, S)
        assert status.tolist() == [0, 0], (name, S)
        assert np.array_equal(rec, want), (name, S)


@pytest.mark.parametrize("name", ["w422_r0", "w422_r3", "w444_r0", "w444_r2"])
def test_huff_kernels_on_damaged_records_equal_the_host_decoder(written, name):
    """The CPU test's damage table in one launch per S: records and status words
    equal the serial host decoder's byte for byte."""
    idx, clean, cases = damaged_records(written, name)
    recs = [clean] + [cases[k] for k in sorted(cases)]
    offs = np.zeros(len(recs) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([r.size for r in recs])
    scans = np.concatenate(recs)
    n = len(recs)
    want, ws = mjpeg.decode_scans_host(scans, offs, n, idx.mw, idx.mh, sampling=idx.sampling)
    assert ws[0] == 0 and (ws < 0).sum() >= 8
    for S in (0,) + SUBSEQ:
        rec, status = huff_gpu(scans, offs, n, idx, S)
        assert status.tolist() == ws.tolist(), (name, S)
        assert np.array_equal(rec, want), (name, S)
    # this sampling's records given to another geometry: refused as a whole
    for other in mjpeg.SAMPLINGS:
        if other != idx.sampling:
            mw, mh, rb = mjpeg.geometry(idx.width, idx.height, other)
            o2 = np.array([0, clean.size], dtype=np.int64)
            rec, status = vops.jpeg_huff(torch.from_numpy(clean).to(DEV), o2, 1, mw, mh,
                                         sampling=other)
            assert mjpeg.status_field(int(status.cpu()[0])) == "scan record"
            assert not rec.cpu().numpy()[384:].any()


# -- decoders end to end -----------------------------------------------------------------------------
@pytest.mark.parametrize("args", [dict(), dict(entropy="gpu", subseq_bytes=0),
                                  dict(entropy="gpu", subseq_bytes=48)],
                         ids=["host", "gpu", "subseq"])
def test_gpu_decoder_against_pils_rgb(args):
    for name in sorted(GOLDEN_CHROMA):
        check_pil_rgb(name, DEV, **args)


@pytest.mark.parametrize("W,H,sampling", [(46, 33, "422"), (45, 33, "444")])
def test_y4m_decoder_against_oracle(tmp_path, W, H, sampling):
    fr = y4m_planes(W, H, 5, 3, sampling)
    path = str(tmp_path / "a.y4m")
    y4m.write_y4m(path, fr, sampling=sampling)
    for filt, (ow, oh) in (("bilinear", (24, 16)), ("antialias", (16, 12))):
        dec = Y4mDecoder(DEV, clip_length=2, height=oh, width=ow, dtype=torch.float32,
                         filter=filt)
        vid, _ = dec.probe(path)
        got = dec.decode(vid, [3, 0]).cpu().numpy()
        for c, s in enumerate((3, 0)):
            y, u, v = (np.stack([fr[s + f][p] for f in range(2)]) for p in range(3))
            ref, _, d, tol = occ.tolerance(y, u, v, ow, oh, None, "bt601", sampling, filt)
            assert tol <= orc.TOL_CEILING
            assert np.abs(got[c][..., :3].astype(np.float64) - ref).max() <= tol


def test_one_gpu_decoder_serves_files_of_every_sampling(written):
    paths = [written[n][0] for n in ("w444_r2", "w422_r0", "w444_7x9", "w422_r3")]
    for args in (dict(), dict(entropy="gpu")):
        one = MjpegDecoder(DEV, clip_length=2, height=20, width=24, dtype=torch.float32, **args)
        ref = MjpegDecoder(CPU, clip_length=2, height=20, width=24, dtype=torch.float32, **args)
        for p in paths + paths[::-1]:
            got = one.decode(one.probe(p)[0], [0])
            one.drain()
            err = (got.cpu() - ref.decode(ref.probe(p)[0], [0])).abs().max().item()
            assert err <= MIRROR_TOL, (p, args, err)


def test_loader_fills_slots_from_a_422_mjpeg_and_a_444_y4m(tmp_path):
    from rnb_amd.models.r2p1d.model import R2P1DLoader
    from rnb_amd.timecard import TimeCard
    (shape,) = R2P1DLoader.output_shape_for(dtype="fp32")
    mpath = str(tmp_path / "a.mjpeg")
    mjpeg.write_mjpeg(mpath, chroma_frames(52, 37, 10, 5, "422"), quality=85, restart_interval=2,
                      sampling="422")
    ypath = str(tmp_path / "b.y4m")
    fr = y4m_planes(45, 33, 10, 8, "444")
    y4m.write_y4m(ypath, fr, sampling="444")
    for backend, path in (("mjpeg", mpath), ("y4m", ypath)):
        loader = R2P1DLoader(DEV, decoder=backend, num_clips_population=[1],
                             num_clips_weights=[1], seed=0, dtype="fp32", warmup=1)
        slot = torch.full(shape, 7.0, device=DEV)
        tc = TimeCard(13)
        (frames,), _, tc = loader.call_into((None,), path, tc, (slot,))
        torch.cuda.synchronize()
        assert tc.num_clips == 1 and frames.data_ptr() == slot.data_ptr()
        assert tuple(frames.shape) == (1,) + tuple(shape[1:]) and torch.all(slot[1:] == 7.0)
        _, starts = tc.extra["clip_src"]
        got = frames.cpu()[0]
        if backend == "mjpeg":
            ref = MjpegDecoder(CPU, dtype=torch.float32)
            want = ref.decode(ref.probe(path)[0], [starts[0]])[0]
            assert (got - want).abs().max().item() <= MIRROR_TOL
        else:
            y, u, v = (np.stack([fr[starts[0] + f][p] for f in range(8)]) for p in range(3))
            ref, _, d, tol = occ.tolerance(y, u, v, 112, 112, None, "bt601", "444")
            assert tol <= orc.TOL_CEILING
            assert np.abs(got.numpy()[..., :3].astype(np.float64) - ref).max() <= tol
