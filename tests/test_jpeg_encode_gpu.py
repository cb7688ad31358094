"""GPU: the JPEG encoder's device stage (memotr_amd/csrc/jpeg_enc.hip: colour launch, FDCT launch) is bit-equal to
the numpy statement of the definition (memotr_amd/data/jpeg_write.py) on every fixture image and both samplings, and
``encode_jpeg`` of a CUDA frame gives Pillow's committed bytes; channel order, batches, pitched rows, a side stream
and the empty batch."""
import numpy as np
import pytest
import torch

from conftest import load_golden

from memotr_amd.data import jpeg_write as JW

pytestmark = pytest.mark.gpu

SUB = {"0": "4:4:4", "2": "4:2:0"}


@pytest.fixture(scope="module")
def enc_lib():
    from memotr_amd.build import build_jpeg_enc_lib
    build_jpeg_enc_lib()
    from memotr_amd import _jpeg_enc_lib
    return _jpeg_enc_lib


@pytest.fixture(scope="module")
def cases():
    return load_golden("jpeg_encode_cases")


def streams(cases):
    off = cases["stream_offsets"]
    for i, name in enumerate(str(n) for n in cases["stream_names"]):
        size, kind, q, s = name.split("_")
        yield name, f"img_{size}_{kind}", int(q[1:]), SUB[s[1:]], cases["streams"][off[i]:off[i + 1]].tobytes()


@pytest.fixture(scope="module")
def host(enc_lib, cases):
    """The host statement's coefficients per (image, quality 75, sampling), computed once."""
    return {(k, sub): JW.forward_coefficients_host(cases[k], 75, sub)
            for k in cases if k.startswith("img_") for sub in ("4:4:4", "4:2:0")}


def test_device_coefficients_equal_the_host_statement_on_every_image(enc_lib, cases, host):
    for (key, sub), want in host.items():
        frame = torch.from_numpy(cases[key]).cuda()
        got = JW.forward_coefficients_device(frame[None], 75, sub)
        n = want.info.coef_count
        assert got.dtype == torch.int16 and tuple(got.shape) == (1, n), (key, sub)
        assert torch.equal(got[0].cpu(), want.flat[:n]), (key, sub)


@pytest.mark.parametrize("quality", [1, 10, 100])
def test_device_coefficients_at_the_ends_of_the_quality_range(enc_lib, cases, quality):
    for key in ("img_31x47_sat", "img_8x9_noise", "img_40x36_smooth"):
        for sub in ("4:4:4", "4:2:0"):
            want = JW.forward_coefficients_host(cases[key], quality, sub)
            got = JW.forward_coefficients_device(torch.from_numpy(cases[key]).cuda()[None], quality, sub)
            assert torch.equal(got[0].cpu(), want.flat[:want.info.coef_count]), (key, sub)


def test_cuda_encode_gives_the_committed_bytes(enc_lib, cases):
    dev = {k: torch.from_numpy(v).cuda() for k, v in cases.items() if k.startswith("img_")}
    for name, key, q, sub, want in streams(cases):
        assert JW.encode_jpeg(dev[key], quality=q, subsampling=sub) == want, name


def test_bgr_on_reversed_channels_gives_the_same_bytes(enc_lib, cases):
    for name, key, q, sub, want in list(streams(cases))[::11]:
        rev = torch.from_numpy(np.ascontiguousarray(cases[key][..., ::-1])).cuda()
        assert JW.encode_jpeg(rev, quality=q, subsampling=sub, bgr=True) == want, name


@pytest.mark.parametrize("sub", ["4:4:4", "4:2:0"])
def test_three_frames_of_one_geometry_in_one_call(enc_lib, cases, host, sub):
    keys = [f"img_31x47_{k}" for k in ("noise", "smooth", "sat")]
    clip = torch.from_numpy(np.stack([cases[k] for k in keys])).cuda()
    got = JW.forward_coefficients_device(clip, 75, sub)
    for i, k in enumerate(keys):
        want = host[(k, sub)]
        assert torch.equal(got[i].cpu(), want.flat[:want.info.coef_count]), k
    s = {"4:4:4": "s0", "4:2:0": "s2"}[sub]
    by_name = {name: data for name, _, _, _, data in streams(cases)}
    assert JW.encode_jpegs(list(clip), threads=2, quality=75, subsampling=sub) == \
        [by_name[f"31x47_{k}_q75_{s}"] for k in ("noise", "smooth", "sat")]


@pytest.mark.parametrize("sub", ["4:4:4", "4:2:0"])
def test_a_pitched_input(enc_lib, cases, host, sub):
    """A column slice of a wider frame: rows are pitched and, from column 5, quads start at every byte alignment."""
    for key in ("img_50x70_noise", "img_17x33_sat"):
        px = cases[key]
        h, w = px.shape[:2]
        wide = torch.randint(0, 256, (h, w + 9, 3), dtype=torch.uint8, device="cuda")
        wide[:, 5:5 + w] = torch.from_numpy(px).cuda()
        view = wide[:, 5:5 + w]
        assert not view.is_contiguous()
        want = host[(key, sub)]
        got = JW.forward_coefficients_device(view[None], 75, sub)
        assert torch.equal(got[0].cpu(), want.flat[:want.info.coef_count]), key
        assert JW.encode_jpeg(view, 75, sub) == JW.huffman_encode(want)


def test_a_non_default_stream(enc_lib, cases, host):
    key = "img_64x96_noise"
    frame = torch.from_numpy(cases[key]).cuda()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = JW.forward_coefficients_device(frame[None], 75, "4:2:0")
    side.synchronize()
    want = host[(key, "4:2:0")]
    assert torch.equal(got[0].cpu(), want.flat[:want.info.coef_count])


def test_an_empty_batch_launches_nothing(enc_lib):
    empty = torch.empty((0, 16, 24, 3), dtype=torch.uint8, device="cuda")
    out = JW.forward_coefficients_device(empty, 75, "4:2:0")
    assert tuple(out.shape) == (0, JW.frame_info(16, 24, "4:2:0").coef_count)
    assert enc_lib.lib.jpegenc_forward_u8(None, 0, 0, None, None, None, 0, None, 0, 0, 0, None) == 0
    assert JW.encode_jpegs([]) == []
