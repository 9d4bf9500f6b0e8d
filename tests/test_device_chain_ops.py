"""The fake (meta) implementations of the device-chain torch ops: shapes and dtypes, no GPU."""
import pytest
import torch


def test_fake_implementations_give_shapes_and_dtypes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from facerecognitionpipeline_amd import torch_ops  # noqa: F401  (registers the ops)
    with FakeTensorMode():
        frames = torch.empty(3, 135, 240, 3, dtype=torch.uint8)
        dets, counts = torch.ops.frhip.detect(frames, 1, 0.5, 8)
        assert (tuple(dets.shape), dets.dtype) == ((3, 8, 15), torch.float32)
        assert (tuple(counts.shape), counts.dtype) == ((3,), torch.int32)
        crops, tforms, ok = torch.ops.frhip.align_detections(frames, dets, counts, 112)
        assert (tuple(crops.shape), crops.dtype) == ((3, 8, 112, 112, 3), torch.uint8)
        assert (tuple(tforms.shape), tforms.dtype) == ((3, 8, 2, 3), torch.float64)
        assert (tuple(ok.shape), ok.dtype) == ((3, 8), torch.uint8)
        blur = torch.ops.frhip.blur_scores(crops.flatten(0, 1))
        assert (tuple(blur.shape), blur.dtype) == ((24,), torch.float64)
    with pytest.raises(ValueError):  # CPU tensors: there is no CPU fallback
        torch.ops.frhip.blur_scores(torch.zeros(1, 8, 8, 3, dtype=torch.uint8))
    with pytest.raises(ValueError):
        torch.ops.frhip.align_detections(torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 2, 15),
                                         torch.zeros(1, dtype=torch.int32), 112)
