"""Pack the reference's Mouse semi-supervised split into the committed fixture
tests/golden/mouse_100_500_0.3/ for machines without the reference tree.

Data only (no reference code): the cached split datasources/temp_data/
Mouse_100_500_0.3.json (semiTrain 100 = 30 labeled + 70 unlabeled, valid 500)
and its 600 PNGs under data/pose/mouse/croppeds_bbox/images, read with PIL and
flipped to BGR (the reference reads them with cv2.imread, utils/process.py:86-88).
The images are grey, so the pack keeps one channel, 20 images per .npz shard
(~20 MB in all, every file under 1 MiB); MouseData.from_pack() restores the
three equal channels.  Run where the reference tree exists:

    python tools/pack_mouse.py <reference tree>
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ubpl-poseestimation_amd"))

from ubpl_amd.mouse import MouseData, DEFAULT_PACK  # noqa: E402


def main(ref):
    src = MouseData(root=os.path.join(ref, "data", "pose", "mouse", "croppeds_bbox"),
                    split_dir=os.path.join(ref, "datasources", "temp_data"))
    src.write_pack(DEFAULT_PACK, 100, 500, 0.3)
    sizes = [os.path.getsize(os.path.join(DEFAULT_PACK, f)) for f in os.listdir(DEFAULT_PACK)]
    print("wrote", DEFAULT_PACK, len(sizes), "files,", sum(sizes) >> 20, "MiB, largest", max(sizes) >> 10, "KiB")


if __name__ == "__main__":
    main(*sys.argv[1:])
