#!/usr/bin/env python3
"""Turns the DATA files the reference's own tests read (/root/reference/test_data, loaded by
srrg2_proslam/tests/fixtures.hpp:555-1152) into the committed fixtures tests/golden/ref_*.npz, and the
hot-path parameter values of its shipped configurations (configurations/*.conf, read with
srrg2_proslam_amd.formats) into tests/golden/ref_conf_hot_path.json.

Run in the build container only (the reference tree does not exist on the GPU box); the tests read the
.npz files, never /root/reference.  What is stored is data: decoded pixels, depth, ground-truth poses and
the sparse disparity ground truth, and the parameter values the `.conf` reader extracts -- no source text
of the reference.

    python tools/make_ref_fixtures.py [/root/reference]

Decoding follows what the reference's fixtures do with OpenCV:
  * KITTI PNGs are 8-bit grayscale already: cv::imread(.., CV_LOAD_IMAGE_GRAYSCALE) returns the bytes
    (fixtures.hpp:1063-1066).
  * ICL / SceneFlow PNGs are RGB: cv::imread(.., GRAYSCALE) lets libpng convert (png_set_rgb_to_gray with
    0.299 / 0.587, i.e. the 15-bit coefficients 9797 / 19234 / 3737, truncating; a pixel with r == g == b keeps
    its value).  tests/test_ref_pins.py shows this choice reproduces the feature counts the reference pins
    on the ICL images (test_feature_extractors.cpp:111-135), which PIL's or cvtColor's weights do not.
  * ICL depth: 16-bit PGM, millimetres (fixtures.hpp:730-740 converts with 1e-3).
"""
import os
import sys

import numpy as np
from PIL import Image

REF = sys.argv[1] if len(sys.argv) > 1 else "/root/reference"
DATA = os.path.join(REF, "test_data")
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")


def gray_u8(path):
    im = Image.open(path)
    if im.mode == "L":
        return np.array(im)
    assert im.mode == "RGB", im.mode
    rgb = np.array(im).astype(np.int64)
    r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
    y = (r * 9797 + g * 19234 + b * 3737) >> 15
    return np.where((r == g) & (g == b), r, y).astype(np.uint8)


def depth_u16(path):
    d = np.array(Image.open(path))
    assert d.min() >= 0 and d.max() < 65536
    return d.astype(np.uint16)


def poses(path):
    p = np.loadtxt(path)
    assert p.shape[1] == 12
    return p.astype(np.float64)


def scene_flow_gt(path):
    """rows of `row col_left row col_right disparity` (fixtures.hpp SceneFlow::SetUp)"""
    return np.loadtxt(path).astype(np.float32)


def conf_hot_path(names=("kitti", "euroc", "icl", "tum")):
    """{config: {group: {key: value}}} as formats.hot_path_params reads it from the shipped .conf files"""
    import json
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from srrg2_proslam_amd import formats
    out = {n: formats.hot_path_params(formats.read_conf(os.path.join(REF, "configurations", n + ".conf"))) for n in names}
    with open(os.path.join(OUT, "ref_conf_hot_path.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def conf_loop(names=("kitti", "euroc", "icl", "tum", "malaga")):
    """{config: loop group} as formats.loop_params reads it from the shipped .conf files (the loop aligner and its verdict)"""
    import json
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from srrg2_proslam_amd import formats
    out = {n: formats.loop_params(formats.read_conf(os.path.join(REF, "configurations", n + ".conf"))) for n in names}
    with open(os.path.join(OUT, "ref_conf_loop.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def conf_place(names=("kitti", "euroc", "icl", "tum", "malaga")):
    """{config: place group} as formats.place_params reads it from the shipped .conf files (the loop detector's candidate search)"""
    import json
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from srrg2_proslam_amd import formats
    out = {n: formats.place_params(formats.read_conf(os.path.join(REF, "configurations", n + ".conf"))) for n in names}
    with open(os.path.join(OUT, "ref_conf_place.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def conf_graph(names=("kitti", "euroc", "icl", "tum", "malaga")):
    """{config: graph group} as formats.graph_params reads it from the shipped .conf files (the global solver of the pose graph)"""
    import json
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from srrg2_proslam_amd import formats
    out = {n: formats.graph_params(formats.read_conf(os.path.join(REF, "configurations", n + ".conf"))) for n in names}
    with open(os.path.join(OUT, "ref_conf_graph.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def conf_graph_lm(names=("kitti", "euroc", "icl", "tum", "malaga")):
    """{config: LM block of the global solver} as formats.graph_lm_params reads it ({} where the file wires Gauss-Newton): settings only"""
    import json
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from srrg2_proslam_amd import formats
    out = {n: formats.graph_lm_params(formats.read_conf(os.path.join(REF, "configurations", n + ".conf"))) for n in names}
    with open(os.path.join(OUT, "ref_conf_graph_lm.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def conf_closure(names=("kitti", "euroc", "icl", "tum", "malaga")):
    """{config: closure-merger group} as formats.closure_merger_params reads it through the tracker slice's pointer: settings only"""
    import json
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from srrg2_proslam_amd import formats
    out = {n: formats.closure_merger_params(formats.read_conf(os.path.join(REF, "configurations", n + ".conf"))) for n in names}
    with open(os.path.join(OUT, "ref_conf_closure.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def conf_split(names=("kitti", "kitti_in_baselink", "euroc", "icl", "tum", "malaga")):
    """{config: splitting-criterion group} as formats.split_params reads it through MultiGraphSLAM3D's pointer: settings only"""
    import json
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from srrg2_proslam_amd import formats
    out = {n: formats.split_params(formats.read_conf(os.path.join(REF, "configurations", n + ".conf"))) for n in names}
    with open(os.path.join(OUT, "ref_conf_split.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def conf_relocalizer(names=("kitti", "kitti_in_baselink", "euroc", "icl", "tum", "malaga")):
    """{config: MultiRelocalizer3D's max_translation and verdict thresholds} as formats.relocalizer_params reads them: settings only"""
    import json
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from srrg2_proslam_amd import formats
    out = {n: formats.relocalizer_params(formats.read_conf(os.path.join(REF, "configurations", n + ".conf"))) for n in names}
    with open(os.path.join(OUT, "ref_conf_relocalizer.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")


def main():
    k = os.path.join(DATA, "kitti")
    np.savez_compressed(
        os.path.join(OUT, "ref_kitti.npz"),
        city_left=np.stack([gray_u8(os.path.join(k, "city", "image_left_%d.png" % i)) for i in range(5)]),
        city_right=np.stack([gray_u8(os.path.join(k, "city", "image_right_%d.png" % i)) for i in range(5)]),
        highway_left=np.stack([gray_u8(os.path.join(k, "highway", "image_left_%d.png" % i)) for i in (274, 275)]),
        highway_right=np.stack([gray_u8(os.path.join(k, "highway", "image_right_%d.png" % i)) for i in (274, 275)]),
        highway_first_index=274)
    # KITTI 00 / 01 ground-truth trajectories (12 floats per line, row-major 3x4); float32 holds the 7 printed digits
    np.savez_compressed(os.path.join(OUT, "ref_kitti_gt.npz"),
                        city=poses(os.path.join(k, "city", "gt.txt")).astype(np.float32),
                        highway=poses(os.path.join(k, "highway", "gt.txt")).astype(np.float32),
                        city_head_f64=poses(os.path.join(k, "city", "gt.txt"))[:8],
                        highway_274_f64=poses(os.path.join(k, "highway", "gt.txt"))[274:276])
    i = os.path.join(DATA, "icl")
    np.savez_compressed(os.path.join(OUT, "ref_icl.npz"),
                        gray=np.stack([gray_u8(os.path.join(i, "image_rgb_%d.png" % n)) for n in (0, 1, 50)]),
                        depth_mm=np.stack([depth_u16(os.path.join(i, "image_depth_%d.pgm" % n)) for n in (0, 1, 50)]),
                        frame_numbers=np.array([0, 1, 50]))
    s = os.path.join(DATA, "scene_flow")
    np.savez_compressed(os.path.join(OUT, "ref_scene_flow.npz"),
                        left=gray_u8(os.path.join(s, "image_left.png")), right=gray_u8(os.path.join(s, "image_right.png")),
                        gt_threshold_10=scene_flow_gt(os.path.join(s, "gt_stereo_matching_threshold-10.txt")),
                        gt_threshold_100=scene_flow_gt(os.path.join(s, "gt_stereo_matching_threshold-100.txt")))
    conf_hot_path()
    conf_loop()
    conf_place()
    conf_graph()
    conf_graph_lm()
    conf_closure()
    conf_split()
    conf_relocalizer()
    for f in sorted(os.listdir(OUT)):
        if f.startswith("ref_"):
            print(f, os.path.getsize(os.path.join(OUT, f)) // 1024, "KiB")


if __name__ == "__main__":
    main()
