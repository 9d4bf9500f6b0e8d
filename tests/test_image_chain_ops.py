"""The mixed-size device chain without a GPU: the fake (meta) implementations of its torch ops, the
refusal of CPU tensors, and the argument checks of ``process_images(gate=)`` /
``match_images(device_chain=)`` that come before any GPU work."""
import numpy as np
import pytest
import torch


def test_fake_implementations_give_shapes_and_dtypes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from facerecognitionpipeline_amd import torch_ops  # noqa: F401  (registers the ops)
    with FakeTensorMode():
        images = [torch.empty(h, w, 3, dtype=torch.uint8) for h, w in ((1080, 1920), (37, 53), (1, 1))]
        dets, counts = torch.ops.frhip.detect_images(images, 1, 0.5, 8)
        assert (tuple(dets.shape), dets.dtype) == ((3, 8, 15), torch.float32)
        assert (tuple(counts.shape), counts.dtype) == ((3,), torch.int32)
        crops, tforms, ok = torch.ops.frhip.align_image_detections(images, dets, counts, 224)
        assert (tuple(crops.shape), crops.dtype) == ((3, 8, 224, 224, 3), torch.uint8)
        assert (tuple(tforms.shape), tforms.dtype) == ((3, 8, 2, 3), torch.float64)
        assert (tuple(ok.shape), ok.dtype) == ((3, 8), torch.uint8)
        assert dets.device == crops.device == images[0].device


def test_cpu_tensors_are_refused():
    from facerecognitionpipeline_amd import torch_ops  # noqa: F401
    image = torch.zeros(8, 8, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="no CPU fallback"):
        torch.ops.frhip.detect_images([image], 1, 0.5, 8)
    with pytest.raises(ValueError, match="no CPU fallback"):
        torch.ops.frhip.align_image_detections([image], torch.zeros(1, 2, 15), torch.zeros(1, dtype=torch.int32), 112)


class _HostDetector:
    """The reference detector's contract and nothing more: no ``model``, no ``detect_images_device``."""

    def detect(self, image):
        return []


def _processor():
    from facerecognitionpipeline_amd.face_recognition import FaceProcessor
    return FaceProcessor(output_size=112, detector=_HostDetector())


def test_process_images_gate_argument():
    fp = _processor()
    image = np.zeros((8, 8, 3), np.uint8)
    for bad in ("gpu", "", None, True):
        with pytest.raises(ValueError, match="gate"):
            fp.process_images([image], gate=bad)
    with pytest.raises(TypeError, match="detect_images_device"):
        fp.process_images([image], gate="device")
    with pytest.raises(TypeError, match="detect_images_device"):  # before an item is looked at
        fp.process_images(["/no/such/file.png"], errors="return", gate="device")


def test_device_chain_images_needs_the_gpu_detector():
    from facerecognitionpipeline_amd.face_recognition import device_chain_images
    fp = _processor()
    with pytest.raises(TypeError, match="detect_images_device"):
        device_chain_images(fp.detector, fp.aligner, fp.quality_filter, [np.zeros((8, 8, 3), np.uint8)])


def test_match_images_device_chain_argument():
    from facerecognitionpipeline_amd.face_matcher import FaceMatcher
    fm = FaceMatcher.__new__(FaceMatcher)  # no embedder, no gallery: the checks come before both
    fm.processor = _processor()
    fm.verbose = False
    image = np.zeros((8, 8, 3), np.uint8)
    for bad in ("yes", 1, None):
        with pytest.raises(ValueError, match="device_chain"):
            fm.match_images([image], device_chain=bad)
        with pytest.raises(ValueError, match="device_chain"):
            fm.match_single_image("/no/such/file.png", device_chain=bad)
    with pytest.raises(TypeError, match="detect_images_device"):
        fm.match_images([image], device_chain=True)
