"""The gfx950 code of the kernels ea_batch_set_frames launches (cross-compiled, no GPU needed; the listing is obtained the
way tests/test_kernel_code_properties.py obtains it): every step of the Laplacian chain has its batched kernel, none of them
has a private segment -- ea_column_local holds two 32-element arrays that must stay in registers, with the frame's address
arithmetic added to the kernel -- and none uses more scratch than the single-frame kernel that runs the same body."""
import os
import re
import subprocess

import pytest

from edge_alignment_amd import build

PKG = os.path.dirname(os.path.dirname(build.LIB))
# step -> source of its kernels; <T>: instantiated for float and double
STEPS = {"ea_blur_gray": "csrc/ea_preprocess.hip", "ea_laplacian_abs": "csrc/ea_preprocess.hip",
         "ea_threshold_median": "csrc/ea_preprocess.hip", "ea_column_local": "csrc/ea_preprocess.hip",
         "ea_column_carry": "csrc/ea_preprocess.hip", "ea_chamfer_row": "csrc/ea_preprocess.hip",
         "ea_dt_store<T>": "csrc/ea_preprocess.hip", "ea_edge_count": "csrc/ea_preprocess.hip",
         "ea_edge_scan": "csrc/ea_preprocess.hip", "ea_edge_scatter<T>": "csrc/ea_preprocess.hip",
         "ea_depth_weights<T>": "csrc/ea_kernels.hip"}


@pytest.fixture(scope="module")
def private_bytes(tmp_path_factory):
    """{(kernel base name, 'f' / 'd' / ''): private segment bytes} of the two sources that hold the chain's kernels"""
    extra = dict(build.SOURCES)
    out_dir = tmp_path_factory.mktemp("frames_code")
    procs = []
    for source in sorted(set(STEPS.values())):
        out = str(out_dir / (os.path.basename(source) + ".s"))
        cmd = ([build._hipcc()] + [f for f in build.FLAGS if f != "-fPIC"] + list(extra[source]) +
               ["-S", "--cuda-device-only", "-o", out, os.path.join(PKG, source)])
        procs.append((out, cmd, subprocess.Popen(cmd, stderr=subprocess.DEVNULL)))
    found = {}
    for out, cmd, pr in procs:
        assert pr.wait() == 0, cmd
        for name, body in re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", open(out).read(), re.S):
            m = re.match(r"_ZN2ea\d+(ea_\w+?_kernel)(?:I([fd])E)?(?:E|v)", name)
            if m:
                found[(m.group(1), m.group(2) or "")] = int(re.search(r"amdhsa_private_segment_fixed_size (\d+)", body).group(1))
    return found


def _kernels_of(step):
    base, types = (step[:-3], ("f", "d")) if step.endswith("<T>") else (step, ("",))
    return [((base + "_frames_kernel", t), (base + "_kernel", t)) for t in types]


@pytest.mark.parametrize("step", sorted(STEPS))
def test_batched_kernel_has_no_private_segment_and_no_more_than_its_single_frame_form(private_bytes, step):
    for batched, single in _kernels_of(step):
        assert batched in private_bytes, (batched, sorted(k for k in private_bytes if "frames" in k[0]))
        assert single in private_bytes, single
        assert private_bytes[batched] == 0, (batched, private_bytes[batched])
        assert private_bytes[batched] <= private_bytes[single], (batched, private_bytes[batched], private_bytes[single])


def test_every_batched_kernel_belongs_to_a_listed_step(private_bytes):
    """a batched kernel added later is checked too, or this fails"""
    listed = {b for step in STEPS for b, _ in _kernels_of(step)}
    assert {k for k in private_bytes if k[0].endswith("_frames_kernel")} == listed
