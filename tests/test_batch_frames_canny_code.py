"""The gfx950 code of the kernels ea_batch_set_frames_canny adds (cross-compiled, no GPU needed; the listing is obtained the
way tests/test_batch_frames_code.py obtains it): every step of the Canny chain has its ea_<step>_batch_kernel beside the
single-frame ea_<step>_kernel that runs the same body, with a private segment no larger than that kernel's -- the hysteresis
holds uint8_t v[64] and two 64-bit masks per lane, which must stay in registers with the frame's address arithmetic added --
and the single-frame kernels, which now call the shared bodies, still have the private segments they had before."""
import os
import re
import subprocess

import pytest

from edge_alignment_amd import build

PKG = os.path.dirname(os.path.dirname(build.LIB))
SOURCE = "csrc/ea_preprocess.hip"
# step -> private segment bytes of its single-frame kernel before the bodies were shared (recorded from that revision's
# listing, same flags, when this test was added)
STEPS = {"ea_boxblur_gray": 0, "ea_sobel_mag": 0, "ea_canny_nms": 0, "ea_canny_hysteresis": 0, "ea_canny_finish": 0}


@pytest.fixture(scope="module")
def private_bytes(tmp_path_factory):
    """{kernel base name: private segment bytes} of the source that holds the chain's kernels"""
    out = str(tmp_path_factory.mktemp("frames_canny_code") / "ea_preprocess.s")
    cmd = ([build._hipcc()] + [f for f in build.FLAGS if f != "-fPIC"] + list(dict(build.SOURCES)[SOURCE]) +
           ["-S", "--cuda-device-only", "-o", out, os.path.join(PKG, SOURCE)])
    assert subprocess.call(cmd, stderr=subprocess.DEVNULL) == 0, cmd
    found = {}
    for name, body in re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", open(out).read(), re.S):
        m = re.match(r"_ZN2ea\d+(ea_\w+?_kernel)(?:I([fd])E)?(?:E|v)", name)
        if m:
            found[m.group(1) + (m.group(2) or "")] = int(re.search(r"amdhsa_private_segment_fixed_size (\d+)", body).group(1))
    return found


@pytest.mark.parametrize("step", sorted(STEPS))
def test_batched_kernel_stands_beside_its_single_frame_kernel_with_no_more_private_memory(private_bytes, step):
    batched, single = step + "_batch_kernel", step + "_kernel"
    assert batched in private_bytes, (batched, sorted(k for k in private_bytes if "batch" in k))
    assert single in private_bytes, single
    assert private_bytes[batched] <= private_bytes[single], (batched, private_bytes[batched], private_bytes[single])


@pytest.mark.parametrize("step", sorted(STEPS))
def test_single_frame_kernel_keeps_its_private_segment(private_bytes, step):
    assert private_bytes[step + "_kernel"] == STEPS[step], (step, private_bytes[step + "_kernel"])


def test_the_new_kernels_are_the_five_batch_kernels_and_none_is_named_as_a_laplacian_one(private_bytes):
    """tests/test_batch_frames_code.py owns the names ending in _frames_kernel: the Canny chain adds none"""
    added = {k for k in private_bytes if k.endswith("_batch_kernel")}
    assert added == {s + "_batch_kernel" for s in STEPS}
    assert not any(k.endswith("_frames_kernel") for k in added)
    assert not any(k.startswith(tuple(STEPS)) and k.endswith("_frames_kernel") for k in private_bytes)
