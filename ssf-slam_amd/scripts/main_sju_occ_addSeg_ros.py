#!/usr/bin/env python3
"""Drop-in for the reference's scripts/ActiveSceneFlow/main_sju_occ_addSeg_ros.py (the `type=` target
of launch/run_Seg_ActiveSceneFlow.launch): the same node, topics and ~DATASET_PATH / ~MODEL_PATH
parameters, with the subsample, the TFlow network, the ground-truth mask (s_fg_mask == 0) and the
float32 Kabsch on the MI355X (ssf.entry.active_scene_flow_main).  Without rospy: --dataset PATH
--model_path CHECKPOINT replays the launch graph offline."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

from ssf.entry import active_scene_flow_main  # noqa: E402

if __name__ == "__main__":
    active_scene_flow_main("main_sju_occ_addSeg_ros.py")
