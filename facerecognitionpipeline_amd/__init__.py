"""MI355X-native (gfx950) face embed + match hot path.

Drop-in for the reference's ``FaceEmbedder`` / ``GalleryManager.search`` /
``FaceMatcher.match_single_face`` seams, backed by hand-written HIP kernels in
``libfrhip.so`` (C ABI: ``include/frhip.h``).  Import is cheap: the GPU
library loads on first use and raises if it is missing — there is no CPU
fallback.
"""
from .arch import block_specs, flop_per_face, state_dict_schema  # noqa: F401

__all__ = ["FaceEmbedder", "GalleryManager", "FaceMatcher", "StudentEnrollment", "SimpleTracker", "FrameAccumulator",
           "CameraFaceCapture", "LiveRecognitionTracker", "LiveFaceRecognition", "DatasetPreprocessor", "ProbeSegmenter",
           "ProbeLabeler", "EmbeddingGenerator", "FaceRecognitionServer", "ServerRecognitionTracker", "create_app",
           "block_specs", "flop_per_face", "state_dict_schema"]


def __getattr__(name):
    if name == "FaceEmbedder":
        from .face_embedder import FaceEmbedder
        return FaceEmbedder
    if name == "GalleryManager":
        from .gallery_manager import GalleryManager
        return GalleryManager
    if name == "FaceMatcher":
        from .face_matcher import FaceMatcher
        return FaceMatcher
    if name == "StudentEnrollment":
        from .enroll_students import StudentEnrollment
        return StudentEnrollment
    if name in ("SimpleTracker", "FrameAccumulator", "CameraFaceCapture"):
        from . import face_detection
        return getattr(face_detection, name)
    if name in ("LiveRecognitionTracker", "LiveFaceRecognition"):
        from . import face_recognition_live
        return getattr(face_recognition_live, name)
    if name == "DatasetPreprocessor":
        from .dataset_preprocessor import DatasetPreprocessor
        return DatasetPreprocessor
    if name == "ProbeSegmenter":
        from .segment_dataset import ProbeSegmenter
        return ProbeSegmenter
    if name == "ProbeLabeler":
        from .probe_labeler import ProbeLabeler
        return ProbeLabeler
    if name == "EmbeddingGenerator":
        from .embedding_generator import EmbeddingGenerator
        return EmbeddingGenerator
    if name in ("FaceRecognitionServer", "create_app"):
        from . import face_recognition_server
        return getattr(face_recognition_server, name)
    if name == "ServerRecognitionTracker":  # the server module's LiveRecognitionTracker: the name is the live loop's here
        from .face_recognition_server import LiveRecognitionTracker
        return LiveRecognitionTracker
    raise AttributeError(name)
