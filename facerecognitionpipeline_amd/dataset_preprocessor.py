"""Drop-in ``DatasetPreprocessor`` (dataset_preprocessor.py): walk a tree of class folders of
photographs, detect and align every face at ``output_size`` 224 and write the crops with
``probe_positive_metadata.json`` -- the input of ``segment_dataset.ProbeSegmenter``.

The reference runs ``FaceProcessor.process_image(path, return_all=True)`` once per photograph.  Here the
walk only lists the photographs, in the reference's order; they are decoded and handed to
``FaceProcessor.process_images`` in chunks of ``batch_size``, so detection, alignment and the blur
scores of a chunk are one batched GPU call each although the photographs differ in size.  The walk
order, the standardised names, the metadata (keys, key order, value types, entry order) and the
per-image error behaviour are the reference's (``tests/golden/dataset_preprocessor.npz``).

Files are decoded by ``load_image_rgb`` and the crops written by PIL at JPEG quality 95 (cv2.imwrite's
default); cv2 is not in the image, and JPEG encoders differ in rounding, so the crop files' bytes are
not pinned to cv2's -- as for ``FaceProcessor.process_image``.
"""
from __future__ import annotations

import argparse
import json
import os
from typing import Dict, List, Optional, Tuple

VALID_EXTENSIONS = {".jpg", ".jpeg", ".png", ".bmp"}
ANGLE_FOLDERS = ["center", "left", "right"]
DEFAULT_QUALITY_CONFIG = {"min_det_score": 0.3, "min_face_size": 30, "max_yaw": 90, "max_pitch": 90, "max_roll": 90,
                          "check_blur": True, "blur_threshold": 100}


class DatasetPreprocessor:
    """The reference's constructor arguments and defaults, plus ``batch_size`` (photographs per
    ``process_images`` call; bounds the host and device memory of a chunk), ``processor`` (a ready
    ``FaceProcessor``, or any object with ``process_images`` or ``process_image``), ``detector_model_path``
    (a SCRFD-10G state dict in ``detector_arch`` keys; without it and without ``processor`` the detector
    runs the seeded synthetic weights, and says so), ``device`` and ``verbose``."""

    def __init__(self, output_size=224, det_size=(640, 640), det_thresh=0.3, quality_filter_config: Optional[Dict] = None,
                 batch_size: int = 32, processor=None, detector_model_path: Optional[str] = None, device=None,
                 verbose: bool = True):
        if batch_size < 1:
            raise ValueError("batch_size must be at least 1")
        self.batch_size = int(batch_size)
        self.verbose = verbose
        if processor is None:
            from .face_recognition import FaceDetector, FaceProcessor
            if detector_model_path is None:
                self._say("No detector weights given (detector_model_path): SCRFD-10G runs seeded synthetic weights")
            detector = FaceDetector(det_size, det_thresh, model_path=detector_model_path, device=device)
            processor = FaceProcessor(output_size=output_size, detector=detector, device=device,
                                      quality_filter_config=dict(quality_filter_config or DEFAULT_QUALITY_CONFIG))
        self.processor = processor

    def _say(self, *a) -> None:
        if self.verbose:
            print(*a)

    def standardize_filename(self, original_path: str, class_id: str, angle: str, image_idx: int) -> str:
        return f"{class_id}_{angle}_{image_idx:03d}.jpg"

    # -- the walk -----------------------------------------------------------------------------
    @staticmethod
    def _images_of(folder: str) -> List[str]:
        return sorted(f for f in os.listdir(folder) if os.path.splitext(f)[1].lower() in VALID_EXTENSIONS)

    def _list_class(self, input_dir: str, class_id: str) -> List[Tuple[str, str, str]]:
        """The photographs of one class folder in the reference's order: (path, angle, standardised
        name without extension).  With any of the ``center`` / ``left`` / ``right`` folders present,
        those folders in that order; otherwise the files of the class folder itself, the angle read
        from the file name ('left', then 'right', else 'center').  ``img_idx`` counts from 1 per folder."""
        class_path = os.path.join(input_dir, class_id)
        jobs = []
        if any(os.path.isdir(os.path.join(class_path, a)) for a in ANGLE_FOLDERS):
            for angle in ANGLE_FOLDERS:
                folder = os.path.join(class_path, angle)
                if not os.path.isdir(folder):
                    self._say(f"Missing angle folder: {angle}")
                    continue
                for idx, name in enumerate(self._images_of(folder), start=1):
                    path = os.path.join(folder, name)
                    jobs.append((path, angle, os.path.splitext(self.standardize_filename(path, class_id, angle, idx))[0]))
        else:
            for idx, name in enumerate(self._images_of(class_path), start=1):
                lower = name.lower()
                angle = "left" if "left" in lower else "right" if "right" in lower else "center"
                path = os.path.join(class_path, name)
                jobs.append((path, angle, os.path.splitext(self.standardize_filename(path, class_id, angle, idx))[0]))
        return jobs

    # -- processing ---------------------------------------------------------------------------
    def _faces_of(self, paths: List[str]) -> List:
        """Per path the processor's face list, or the exception that image ran into."""
        from .face_recognition import load_image_rgb
        if not hasattr(self.processor, "process_images"):  # a per-image processor
            out = []
            for p in paths:
                try:
                    out.append(self.processor.process_image(p, return_all=True))
                except Exception as e:
                    out.append(e)
            return out
        out: List = [None] * len(paths)
        images, slots = [], []
        for i, p in enumerate(paths):
            image = load_image_rgb(p)
            if image is None:
                out[i] = ValueError(f"Could not load image: {p}")
            else:
                images.append(image)
                slots.append(i)
        try:
            results = self.processor.process_images(images, return_all=True, errors="return") if images else []
        except (ValueError, NotImplementedError):
            # the library refused one image's arguments (a side out of range, too small to letterbox) or
            # met its 4096-anchor limit: image by image, so only that one is lost.  Anything else -- a
            # device error above all -- is raised: nothing more is launched after it.
            results = []
            for image in images:
                try:
                    results.append(self.processor.process_images([image], return_all=True, errors="return")[0])
                except (ValueError, NotImplementedError) as e:
                    results.append(e)
        for i, r in zip(slots, results):
            out[i] = r
        return out

    def _save_faces(self, faces, image_path: str, class_id: str, angle: str, standardized_name: str, output_dir: str,
                    metadata_list: List[Dict]) -> int:
        from PIL import Image
        original = os.path.basename(image_path)
        self._say(f"  Processing: {original} -> {standardized_name}")
        try:
            if isinstance(faces, Exception):
                raise faces
            if len(faces) == 0:
                self._say("No faces detected")
                return 0
            saved = 0
            for k, face in enumerate(faces):
                name = f"{standardized_name}_face{k}.jpg"
                Image.fromarray(face["aligned_face"]).save(os.path.join(output_dir, name), quality=95)
                m = face["quality_metrics"]
                metadata_list.append({
                    "filename": name,
                    "class_id": class_id,
                    "source_image": original,
                    "standardized_name": f"{standardized_name}.jpg",
                    "face_index": k,
                    "angle": angle,
                    "det_score": float(face["det_score"]),
                    "yaw": float(m.get("yaw", 0.0)),
                    "pitch": float(m.get("pitch", 0.0)),
                    "roll": float(m.get("roll", 0.0)),
                    "blur_score": float(m.get("blur_score", 0.0)),
                    "face_size": int(m.get("face_size", 0)),
                    "bbox": face["bbox"].tolist(),
                })
                self._say(f"Face {k}: det={face['det_score']:.3f}, blur={m.get('blur_score', 0):.0f}, "
                          f"yaw={m.get('yaw', 0):.1f}, pitch={m.get('pitch', 0):.1f} -> {name}")
                saved += 1
            return saved
        except Exception as e:  # the reference's per-image try / except: 0 faces, and the walk goes on
            self._say(f"    Error: {e}")
            return 0

    def process_single_image(self, image_path: str, class_id: str, angle: str, standardized_name: str, output_dir: str,
                             metadata_list: List[Dict]) -> int:
        faces = self._faces_of([image_path])[0]
        return self._save_faces(faces, image_path, class_id, angle, standardized_name, output_dir, metadata_list)

    def process_dataset(self, input_dir: str, output_dir: str, probe_dir_name: str = "probe_positive",
                        metadata_filename: str = "probe_positive_metadata.json"):
        probe_dir = os.path.join(output_dir, probe_dir_name)
        os.makedirs(probe_dir, exist_ok=True)
        class_dirs = sorted(d for d in os.listdir(input_dir) if os.path.isdir(os.path.join(input_dir, d)))
        if not class_dirs:
            self._say("No class directories found!")
            return
        jobs = []  # (path, class_id, angle, standardised name), in walk order
        for class_id in class_dirs:
            mine = self._list_class(input_dir, class_id)
            self._say(f"Class {class_id}: {len(mine)} images")
            jobs += [(path, class_id, angle, name) for path, angle, name in mine]
        all_metadata: List[Dict] = []
        total_faces = 0
        for at in range(0, len(jobs), self.batch_size):
            chunk = jobs[at:at + self.batch_size]
            faces = self._faces_of([j[0] for j in chunk])
            for (path, class_id, angle, name), f in zip(chunk, faces):
                total_faces += self._save_faces(f, path, class_id, angle, name, probe_dir, all_metadata)
        metadata_path = os.path.join(output_dir, metadata_filename)
        with open(metadata_path, "w") as f:
            json.dump(all_metadata, f, indent=2)
        self._say(f"Total classes processed: {len(class_dirs)}")
        self._say(f"Total images processed: {len(jobs)}")
        self._say(f"Total faces detected: {total_faces}")
        self._say(f"Average faces per image: {total_faces / max(len(jobs), 1):.2f}")
        self._say(f"Probe images saved to: {probe_dir}\nMetadata saved to: {metadata_path}")
        angles: Dict[str, int] = {}
        for entry in all_metadata:
            angles[entry["angle"]] = angles.get(entry["angle"], 0) + 1
        for angle, count in sorted(angles.items()):
            self._say(f"  {angle}: {count} faces")


def build_parser() -> argparse.ArgumentParser:
    """The reference's command line (dataset_preprocessor.py), plus ``--batch_size`` and ``--detector_model``."""
    p = argparse.ArgumentParser(description="Preprocess classroom dataset for face recognition evaluation")
    p.add_argument("--input_dir", type=str, default="samples/classroom",
                   help="Input directory containing class subdirectories")
    p.add_argument("--output_dir", type=str, default="output/preprocessed", help="Output directory for processed data")
    p.add_argument("--probe_dir", type=str, default="probe_positive", help="Name of subdirectory for probe images")
    p.add_argument("--metadata_file", type=str, default="probe_positive_metadata.json",
                   help="Name of metadata JSON file")
    p.add_argument("--output_size", type=int, default=224, help="Size of aligned face output")
    p.add_argument("--det_thresh", type=float, default=0.3, help="Detection threshold (lower = more detections)")
    p.add_argument("--batch_size", type=int, default=32, help="Photographs per batched GPU call")
    p.add_argument("--detector_model", type=str, default=None,
                   help="SCRFD-10G state dict (detector_arch keys); default: seeded synthetic weights")
    return p


def main(argv=None, processor=None):
    args = build_parser().parse_args(argv)
    pre = DatasetPreprocessor(output_size=args.output_size, det_thresh=args.det_thresh, batch_size=args.batch_size,
                              processor=processor, detector_model_path=args.detector_model)
    pre.process_dataset(input_dir=args.input_dir, output_dir=args.output_dir, probe_dir_name=args.probe_dir,
                               metadata_filename=args.metadata_file)


if __name__ == "__main__":
    main()
