"""Derives the box fields of an Omni3D annotation file on the device (`cubercnn.data.annotate.annotate_dataset`: bbox3D_cam,
bbox2D_proj, bbox2D_trunc, truncation, behind_camera, visibility from center_cam / dimensions / R_cam, K and the image size) and
prints how many annotations each field was written to.  Present fields are kept unless --overwrite is given.
    python tools/annotate_dataset.py IN.json OUT.json [--overwrite]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from omni3d_amd.cubercnn.data.annotate import annotate_dataset  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--overwrite", action="store_true", help="replace derived fields that are already there")
    ap.add_argument("--min-z", type=float, default=0.20, help="a vertex at z <= MIN_Z counts as behind the camera")
    ap.add_argument("--zplane", type=float, default=0.05, help="near plane of the visibility cast")
    args = ap.parse_args(argv)
    with open(args.input) as f:
        dataset = json.load(f)
    counts = annotate_dataset(dataset, overwrite=args.overwrite, min_z=args.min_z, zplane=args.zplane)
    with open(args.output, "w") as f:
        json.dump(dataset, f)
    print("%d images, %d annotations; fields written: %s" % (len(dataset["images"]), len(dataset["annotations"]),
                                                            ", ".join("%s %d" % kv for kv in counts.items())))


if __name__ == "__main__":
    main()
