"""CPU: the public surface of the captured tracker and the captured sequence step (no device needed)."""
import inspect

import pytest

from ratrack_amd import track_train as TT, tracker as T
from ratrack_amd.track4d import Args, Track4D


def test_batched_tracker_takes_the_capture_arguments():
    params = inspect.signature(T.BatchedTracker.__init__).parameters
    for name, default in (("static_state", False), ("graph", False), ("graph_warmup", 2), ("engine", None)):
        assert name in params and params[name].default == default, name
    assert isinstance(T.BatchedTracker.captured, property)


def test_tracker_pipeline_exists_and_takes_groups_and_streams():
    params = list(inspect.signature(T.TrackerPipeline.__init__).parameters)
    assert params[:4] == ["self", "net", "groups", "streams"] and "max_objects" in params
    assert list(inspect.signature(T.TrackerPipeline.submit).parameters)[:6] == ["self", "g", "pc1", "pc2", "feature1", "feature2"]
    assert callable(T.TrackerPipeline.drain) and T.TrackerPipeline.MAX_GROUPS == 4


def test_a_captured_sequence_step_needs_the_model_on_the_gpu():
    with pytest.raises(ValueError, match="graph=True") as e:
        TT.SequenceTrainer(Track4D(Args()), streams=4, graph=True)
    assert "GPU" in str(e.value)
