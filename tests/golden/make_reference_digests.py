"""Record the digests of tests/golden/reference_digests.json from the REFERENCE's own code (oracle/_ref).

    python tests/golden/make_reference_digests.py        # needs the reference tree, so that oracle/_ref is built

Runs the port-vs-reference tests with the live reference in record mode (tests/golden/recorded_reference.py): each
test still asserts that the port equals the reference bit for bit, and stores the digest of the reference's arrays.
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
from oracle import pyoracle as O  # noqa: E402
from recorded_reference import PATH, RECORD_ENV  # noqa: E402

TESTS = [
    "tests/test_oracle.py::test_voxelize_port_equals_reference",
    "tests/test_oracle.py::test_iou_nms_port_equals_reference",
    "tests/test_oracle.py::test_iou_degenerate_pairs",
    "tests/test_oracle.py::test_iou_nms_port_equals_reference_on_box_families",
    "tests/test_oracle.py::test_decode_port_equals_reference",
    "tests/test_oracle.py::test_bev_pool_port_equals_reference",
    "tests/test_oracle.py::test_hard_voxelize_float64_port_equals_ref",
    "tests/test_ssd_golden.py::test_post_process_restatement",
]


def main():
    O.build(ref=True)
    assert O.have_ref(), "oracle/_ref could not be built (is the reference tree present?)"
    if os.path.exists(PATH):
        os.remove(PATH)
    env = dict(os.environ, **{RECORD_ENV: "1"})
    subprocess.check_call([sys.executable, "-m", "pytest", "-q", "-p", "no:cacheprovider", *TESTS], cwd=ROOT, env=env)
    print(PATH, os.path.getsize(PATH), "bytes")


if __name__ == "__main__":
    main()
