"""The splitting criterion's settings: the .conf reader, the values recorded from the six shipped files and configs.py."""
import json
import os

import pytest

from srrg2_proslam_amd import configs, formats, ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_conf_split.json")

# the wiring of the shipped files, with values of its own: the SLAM record points at the criterion by id
CONF = """
"LocalMapSplittingCriterionViewpoint3D" {
  "#id" : 40,
  // rotation difference between the center of the local maps (in radians)
  "local_map_angle_distance_radians" : 0.75,
  "local_map_distance" : 2.5
 }

"LocalMapSplittingCriterionViewpoint3D" {
  "#id" : 41,
  "local_map_angle_distance_radians" : 9,
  "local_map_distance" : 99
 }

"MultiGraphSLAM3D" {
  "#id" : 1,
  "name" : "slam",
  "splitting_criterion" : {
    "#pointer" : 40
   }
 }
"""


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_split_params_follows_the_slam_record_s_pointer():
    got = formats.split_params(formats.parse_conf(CONF))
    assert got == {"class": "LocalMapSplittingCriterionViewpoint3D", "local_map_distance": 2.5, "local_map_angle_distance_radians": 0.75}
    assert formats.split_params(formats.parse_conf('"MultiGraphSLAM3D" { "#id" : 1 }')) == {}


def test_recorded_values_of_the_six_shipped_files(golden):
    assert sorted(golden) == ["euroc", "icl", "kitti", "kitti_in_baselink", "malaga", "tum"]
    for name, group in golden.items():
        assert group["class"] == "LocalMapSplittingCriterionViewpoint3D", name
    assert golden["kitti_in_baselink"] == golden["malaga"] == golden["kitti"]


@pytest.mark.parametrize("name", ["kitti", "euroc", "icl", "tum"])
def test_configs_carry_the_shipped_values(golden, name):
    mine = configs.get(name)["split"]
    group = {k: v for k, v in golden[name].items() if k != "class"}
    assert mine == group
    p = ops.session_params(mine)
    assert (p.split_information, p.lost_information) == (1.0, pytest.approx(0.1, rel=1e-7))
    assert p.local_map_distance == group["local_map_distance"]
