"""``nv12_clip_kernel`` and all four instances of ``yuv420_clip_kernel`` against
the independent fp64 oracle of ``decode_oracle.py`` directly (not via the CPU
mirrors), the bf16 outputs bit for bit, the three reference-free properties,
and ``MjpegDecoder`` on the GPU against PIL's RGB. Cases, inputs and bounds are
those of ``test_decode_oracle_cpu.py``; run with ``-s`` for the figures."""
import pytest
import torch

import decode_oracle as orc
from test_decode_oracle_cpu import (PATH_IDS, PATHS, check_anchor_colours, check_case,
                                    check_chroma_ramp, check_luma_ramp, check_pil_rgb,
                                    check_table)
from test_mjpeg_cpu import GOLDEN_STREAMS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
RESIZE_IDS = ["crop_24x16", "full_31x19"]


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", [c[0] for c in orc.NV12_CASES])
def test_nv12_kernel_against_oracle(name, bf16):
    check_case("nv12", name, DEV, bf16)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", [c[0] for c in orc.YUV420_CASES])
def test_yuv420_kernel_against_oracle(name, bf16):
    """<= 32 clips: the kernel-argument instances (bt601 and jfif)."""
    check_case("yuv420", name, DEV, bf16)


@pytest.mark.parametrize("matrix", ["bt601", "jfif"])
def test_yuv420_kernel_device_offset_table(matrix):
    """33 clips: the FROM_ARRAY instances, ``offs[clip]`` from device memory."""
    check_table(matrix, DEV)


@pytest.mark.parametrize("resize", orc.RAMP_RESIZES, ids=RESIZE_IDS)
@pytest.mark.parametrize("path", PATHS, ids=PATH_IDS)
def test_kernel_luma_ramp(path, resize):
    check_luma_ramp(path, resize, DEV)


@pytest.mark.parametrize("resize", orc.RAMP_RESIZES, ids=RESIZE_IDS)
@pytest.mark.parametrize("path", PATHS, ids=PATH_IDS)
def test_kernel_chroma_ramp(path, resize):
    check_chroma_ramp(path, resize, DEV)


@pytest.mark.parametrize("path", PATHS, ids=PATH_IDS)
def test_kernel_anchor_colours(path):
    check_anchor_colours(path, DEV)


@pytest.mark.parametrize("entropy", ["host", "gpu"])
@pytest.mark.parametrize("name", sorted(GOLDEN_STREAMS))
def test_gpu_decoder_against_pils_rgb(name, entropy):
    check_pil_rgb(name, DEV, entropy=entropy)
