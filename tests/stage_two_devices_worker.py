"""
Child process of tests/test_gpu_stage_sweep.py::test_large_lds_launches_on_two_devices: in ONE process, the two kernels that
raise their dynamic-LDS limit run on device 0 and then on device 1, and both must match the reference on both.
Prints TWO_DEVICES_OK on success.
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (HERE, os.path.join(ROOT, "oracle"), ROOT):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import pnyolo_pkg  # noqa: E402

pnyolo_pkg.load()
import stage_ref as sr  # noqa: E402
from pixel_nerf_yolo_amd import util as putil  # noqa: E402


def main():
    assert torch.cuda.device_count() >= 2
    boxes, iou_t, conf_t = sr.nms_cases()["cluster%d" % sr.NMS_MAX]
    ref_kept, ref_hi, ref_above = sr.nms_fast(boxes, iou_t, conf_t)
    kc, kf, kfd = 1024, 512, 256
    c = sr.fine_case(5, kc, kf, kfd, 0, "bump")
    z_ref = sr.fine_ref(c, kc, kf, kfd, 0, sr.F64)
    for d in (0, 1):
        device = "cuda:%d" % d
        with torch.cuda.device(d):
            b = torch.as_tensor(boxes, device=device)
            kept, hi, above = putil.nms(b, iou_t, conf_t, as_tensor=True)
            assert above == ref_above and np.float32(hi) == np.float32(ref_hi), device
            assert np.array_equal(kept.cpu().numpy(), ref_kept), "nms differs on " + device
            zo = sr.hip_fine(c, kc, kf, kfd, 0, device=device)
            e = sr.err(zo, z_ref)
            assert e <= sr.FINE_BAR, "sample_fine on %s: %.3e" % (device, e)
            print("device %d: nms %d survivors, sample_fine max |err| %.2e" % (d, kept.shape[0], e))
    print("TWO_DEVICES_OK")


if __name__ == "__main__":
    main()
