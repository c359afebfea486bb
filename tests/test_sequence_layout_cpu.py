"""The sequence modules' layout: every name callers import from splatam_amd.sequence is the object of its home
module, and the two graph scorers of splatam_amd.fisher inherit their calls from one base."""
import importlib

import pytest

HOMES = {
    "SlamSequence": "sequence", "PerFrameSlam": "perframe", "ViewScorer": "seqscore",
    "pad_map": "padded_map", "compact_static": "padded_map", "init_map_literal": "padded_map",
    "densify_static": "padded_map",
    "initialize_camera_pose": "frame_ops", "non_presence_mask": "frame_ops", "add_new_gaussians_literal": "frame_ops",
    "add_new_gaussians_device": "frame_ops", "render_depth_sil": "frame_ops", "frame_pointcloud": "frame_ops",
    "_SequenceBase": "capture", "_check_policy": "capture",
}


@pytest.mark.parametrize("name", sorted(HOMES))
def test_sequence_reexports_the_home_modules_object(name):
    from splatam_amd import sequence
    home = importlib.import_module("splatam_amd." + HOMES[name])
    assert name in sequence.__all__
    assert getattr(sequence, name) is getattr(home, name)
    assert getattr(home, name).__module__ == home.__name__  # (defined there, not passed on)


def test_sequence_all_is_the_list():
    from splatam_amd import sequence
    assert sorted(sequence.__all__) == sorted(HOMES)


def test_graph_scorers_inherit_their_calls():
    from splatam_amd.fisher import BatchedFisher, SequenceFisher
    shared = ("_load", "hessian_sum", "scores", "_replay_scores", "gains", "overflowed")
    for cls in (BatchedFisher, SequenceFisher):
        for name in shared:
            assert name not in cls.__dict__ and callable(getattr(cls, name)), (cls.__name__, name)
    for name in shared:
        assert getattr(BatchedFisher, name) is getattr(SequenceFisher, name)
