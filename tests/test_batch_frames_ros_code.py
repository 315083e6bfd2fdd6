"""The gfx950 code of the kernels ea_batch_set_frames_ros adds (cross-compiled, no GPU needed; the listing is obtained the
way tests/test_batch_frames_code.py obtains it): each step the ROS chain does not share with the other two -- the 3-channel
L2 Sobel, the exact-EDT row pass, the store from the float distance, the ROS scatter, the two halving steps -- has its
ea_<step>_stack_kernel beside the single-frame ea_<step>_kernel that runs the same body, with a private segment no larger
than that kernel's, and the single-frame kernels, which now call the shared bodies, still have the private segments they
had before.  The row pass is the one to watch: 64-bit squared distances and the winning (dx, dy) pair per lane, with the
frame's address arithmetic and the slot's early exit added."""
import os
import re
import subprocess

import pytest

from edge_alignment_amd import build

PKG = os.path.dirname(os.path.dirname(build.LIB))
SOURCE = "csrc/ea_preprocess.hip"
# step (<T>: instantiated for float and double) -> private segment bytes of its single-frame kernel before the bodies were
# shared (recorded from that revision's listing, same flags, when this test was added)
STEPS = {"ea_sobel_mag_l2_bgr": 0, "ea_edt_row": 0, "ea_dt_store<T>": 0, "ea_edge_scatter_ros<T>": 0, "ea_resize_half_bgr8": 0,
         "ea_resize_half_f32": 0}


@pytest.fixture(scope="module")
def private_bytes(tmp_path_factory):
    """{(kernel base name, 'f' / 'd' / ''): private segment bytes} of the source that holds the chain's kernels"""
    out = str(tmp_path_factory.mktemp("frames_ros_code") / "ea_preprocess.s")
    cmd = ([build._hipcc()] + [f for f in build.FLAGS if f != "-fPIC"] + list(dict(build.SOURCES)[SOURCE]) +
           ["-S", "--cuda-device-only", "-o", out, os.path.join(PKG, SOURCE)])
    assert subprocess.call(cmd, stderr=subprocess.DEVNULL) == 0, cmd
    found = {}
    for name, body in re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", open(out).read(), re.S):
        m = re.match(r"_ZN2ea\d+(ea_\w+?_kernel)(?:I([fd])E)?(?:E|v)", name)
        if m:
            found[(m.group(1), m.group(2) or "")] = int(re.search(r"amdhsa_private_segment_fixed_size (\d+)", body).group(1))
    return found


def _kernels_of(step):
    base, types = (step[:-3], ("f", "d")) if step.endswith("<T>") else (step, ("",))
    return [((base + "_stack_kernel", t), (base + "_kernel", t)) for t in types]


@pytest.mark.parametrize("step", sorted(STEPS))
def test_stack_kernel_stands_beside_its_single_frame_kernel_with_no_more_private_memory(private_bytes, step):
    for stacked, single in _kernels_of(step):
        assert stacked in private_bytes, (stacked, sorted(k for k in private_bytes if "stack" in k[0]))
        assert single in private_bytes, single
        assert private_bytes[stacked] <= private_bytes[single], (stacked, private_bytes[stacked], private_bytes[single])


@pytest.mark.parametrize("step", sorted(STEPS))
def test_single_frame_kernel_keeps_its_private_segment(private_bytes, step):
    for _, single in _kernels_of(step):
        assert private_bytes[single] == STEPS[step], (single, private_bytes[single])


def test_the_stack_kernels_are_exactly_the_new_ones(private_bytes):
    """tests/test_batch_frames_code.py owns the names ending in _frames_kernel, tests/test_batch_frames_canny_code.py those
    ending in _batch_kernel: the ROS chain adds to neither, and a stack kernel added later is checked here or this fails"""
    listed = {k for step in STEPS for k, _ in _kernels_of(step)}
    assert {k for k in private_bytes if k[0].endswith("_stack_kernel")} == listed
    bases = tuple(s[:-3] if s.endswith("<T>") else s for s in STEPS)
    assert not any(k[0].startswith(bases) and k[0].endswith(("_frames_kernel", "_batch_kernel")) and k[0] != "ea_dt_store_frames_kernel"
                   for k in private_bytes)
