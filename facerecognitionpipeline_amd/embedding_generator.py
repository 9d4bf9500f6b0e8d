"""Drop-in ``embedding_generator`` (embedding_generator.py): from the enrollment folders and the labelled
probe crops to the ``.pkl`` / ``.json`` dicts ``evaluate_models.load_embeddings`` reads -- the four
galleries (one-shot / few-shot x base / augmented), the probe sets (unsegmented, ten segments,
negatives) and ``generation_summary.json``.

Mirrors the reference class: constructor arguments, method names, return dicts, file names and
printed warnings.  What changes is how the work is batched:

* ``process_gallery_enrollment`` hands the photographs of ALL persons to one
  ``FaceProcessor.process_images`` call and all kept crops to one augment + embed pass
  (``enroll_students.embed_augmented``); the reference detects and embeds person by person.  Within
  one ``generate_all_embeddings`` the augmented pass of an enrollment type reuses the crops of its
  base pass (same files, same call), so every photograph is detected twice less.
* the probe methods decode ``block_images`` files at a time on the host and embed each block through
  ``FaceEmbedder.embed_images`` -- one library call for crops of any mix of sizes (the reference runs
  one ``cv2.resize`` and one ``extract_embedding`` per file).

Files are decoded by ``load_image_rgb`` (PIL; cv2 is not in the image), as everywhere in this package.
"""
from __future__ import annotations

import argparse
import json
import pickle
from datetime import datetime
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np

from .enroll_students import _check_count, _sliced_count, augment_face_for_enrollment, embed_augmented

PROJECT_ROOT = Path(__file__).resolve().parent.parent.parent  # embedding_generator.py:18-22
SEGMENT_CATEGORIES = ["high_quality", "blur_blurry", "blur_sharp", "face_large", "face_medium", "face_small",
                      "pose_easy", "pose_medium", "pose_hard", "low_quality"]
GALLERY_AUGMENTATIONS = 8  # embedding_generator.py:177


def _image_files(folder: Path) -> List[Path]:
    """The reference's listing: case-sensitive ``*.jpg``, ``*.png``, ``*.jpeg`` (no ``.bmp``), sorted."""
    return sorted(list(folder.glob("*.jpg")) + list(folder.glob("*.png")) + list(folder.glob("*.jpeg")))


class EmbeddingGenerator:
    def __init__(self, model_type="adaface", architecture="ir_101", dataset_root=None, output_root=None, *,
                 face_processor=None, embedder=None, device=None, verbose=True, block_images: int = 1024):
        """The reference's arguments and defaults.  ``face_processor`` and ``embedder`` inject existing
        objects instead of building the reference's defaults; ``device`` is the HIP device of the ones
        built here; ``block_images`` is how many probe files are decoded and embedded at a time (it
        bounds the host and device memory of the probe methods)."""
        if block_images < 1:
            raise ValueError("block_images must be at least 1")
        self.model_type = model_type
        self.architecture = architecture
        self.model_name = f"{model_type}_{architecture}"
        self.verbose = verbose
        self.block_images = int(block_images)
        self.dataset_root = PROJECT_ROOT / "dataset" if dataset_root is None else Path(dataset_root)
        self.output_root = PROJECT_ROOT / "output" / "v0" if output_root is None else Path(output_root)

        self._print(f"\n{'=' * 60}")
        self._print("Initializing Embedding Generator")
        self._print(f"Model: {self.model_name}")
        self._print(f"{'=' * 60}\n")

        if embedder is None:
            from .face_embedder import FaceEmbedder
            embedder = FaceEmbedder(architecture=architecture, model_type=model_type, device=device)
        self.embedder = embedder
        if face_processor is None:
            from .face_recognition import FaceProcessor
            face_processor = FaceProcessor(
                output_size=112, det_size=(640, 640), det_thresh=0.5,
                quality_filter_config={"min_det_score": 0.5, "min_face_size": 40},
                providers=["CUDAExecutionProvider", "CPUExecutionProvider"], device=device)
        self.face_processor = face_processor
        self._crop_cache: Optional[Dict[str, list]] = None  # per enrollment type, inside generate_all_embeddings

        self.output_dir = self.output_root / "embeddings" / self.model_name
        self.output_dir.mkdir(parents=True, exist_ok=True)
        self._print(f"Embeddings will be saved to: {self.output_dir}\n")

    def _print(self, *args, **kw) -> None:
        if self.verbose:
            print(*args, **kw)

    # -- reference helpers ---------------------------------------------------------------------
    def extract_name_from_filename(self, filename: str) -> str:
        parts = Path(filename).stem.split("_")
        name_parts = []
        for part in parts:
            if part.isdigit():
                break
            name_parts.append(part)
        return "_".join(name_parts) if name_parts else parts[0]

    def save_embeddings_json(self, data: Dict, output_path: Path):
        def convert_to_serializable(obj):
            if isinstance(obj, np.ndarray):
                return obj.tolist()
            if isinstance(obj, dict):
                return {key: convert_to_serializable(value) for key, value in obj.items()}
            if isinstance(obj, list):
                return [convert_to_serializable(item) for item in obj]
            if isinstance(obj, (np.int64, np.int32)):
                return int(obj)
            if isinstance(obj, (np.float64, np.float32)):
                return float(obj)
            return obj

        json_path = Path(output_path).with_suffix(".json")
        with open(json_path, "w") as f:
            json.dump(convert_to_serializable(data), f, indent=2)
        self._print(f"JSON saved to: {json_path}")

    def load_image(self, image_path: Path) -> np.ndarray:
        from .face_recognition import load_image_rgb
        img = load_image_rgb(str(image_path))
        if img is None:
            raise ValueError(f"Failed to load image: {image_path}")
        return img

    # -- the device passes ---------------------------------------------------------------------
    def _faces_of(self, paths: List[str]) -> List:
        """Per path the processor's face list (``return_all=True``), or the exception that file ran into."""
        if not paths:
            return []
        if hasattr(self.face_processor, "process_images"):
            return list(self.face_processor.process_images(paths, return_all=True, errors="return"))
        out = []
        for p in paths:  # a per-image processor
            try:
                out.append(self.face_processor.process_image(p, return_all=True))
            except Exception as e:
                out.append(e)
        return out

    def _embed_gallery(self, crops: List[np.ndarray], copies: int) -> np.ndarray:
        """``copies`` augmented copies of every crop (1: the crops themselves), embedded with
        ``normalize=True`` -> float32 [len(crops) * copies, 512], crop-major."""
        from . import _lib
        model = getattr(self.embedder, "model", None)
        if isinstance(model, _lib.Handle):  # (variant 0 of the augmentation is the crop itself)
            return embed_augmented(self.embedder, model, self.embedder.device, crops, copies)
        # an injected embedder without a library handle: the reference's list, built crop by crop
        faces = [v for c in crops for v in (augment_face_for_enrollment(c, copies) if copies > 1 else [c])]
        return np.asarray(self.embedder.extract_embeddings_batch(faces, normalize=True), dtype=np.float32)

    def _embed_files(self, files: List[Path]):
        """Decode and embed ``files`` in blocks of ``block_images``: yields (path, float32 [512]) for every
        file that decodes, in order; an undecodable file is printed and skipped."""
        for at in range(0, len(files), self.block_images):
            kept, images = [], []
            for path in files[at:at + self.block_images]:
                try:
                    images.append(self.load_image(path))
                    kept.append(path)
                except Exception as e:
                    self._print(f"Error processing {path.name}: {e}")
            if not kept:
                continue
            emb = self.embedder.embed_images(images, normalize=True)
            emb = np.asarray(emb.cpu().numpy() if hasattr(emb, "cpu") else emb, dtype=np.float32)
            yield from zip(kept, emb)

    # -- reference API -------------------------------------------------------------------------
    def process_gallery_enrollment(self, enrollment_type: str = "one-shot", use_augmentation: bool = False) -> Dict:
        self._print(f"\n{'=' * 60}")
        suffix = "augmented" if use_augmentation else "base"
        self._print(f"Processing Gallery: {enrollment_type}-{suffix}")
        self._print(f"{'=' * 60}\n")

        gallery_dir = self.dataset_root / "enrollment" / enrollment_type
        if not gallery_dir.exists():
            self._print(f"Warning: Gallery directory not found: {gallery_dir}")
            return {}

        # (person, [(file name, crop)]) per person with image files, in the reference's order
        persons = None if self._crop_cache is None else self._crop_cache.get(enrollment_type)
        if persons is None:
            persons = self._collect_enrollment(gallery_dir)
            if self._crop_cache is not None:
                self._crop_cache[enrollment_type] = persons
        else:
            self._print(f"Reusing the aligned crops of the {enrollment_type} base pass")

        copies = _sliced_count(GALLERY_AUGMENTATIONS) if use_augmentation else 1
        _check_count(copies)
        crops = [crop for _person, kept in persons for _name, crop in kept]
        allemb = self._embed_gallery(crops, copies) if crops else np.zeros((0, 512), np.float32)

        gallery_embeddings = {}
        row = 0
        for person_name, kept in persons:
            if not kept:
                continue
            n = len(kept) * copies
            embeddings = np.ascontiguousarray(allemb[row:row + n])
            row += n
            valid_files = [name for name, _crop in kept]
            gallery_embeddings[person_name] = {
                "embeddings": embeddings,
                "num_images": len(valid_files),
                "num_embeddings": len(embeddings),
                "image_files": valid_files,
                "enrollment_type": enrollment_type,
                "augmented": use_augmentation,
            }
            self._print(f"  {person_name}: {len(embeddings)} embeddings from {len(valid_files)} images")

        self._print(f"\nTotal persons enrolled: {len(gallery_embeddings)}")
        output_path = self.output_dir / f"gallery_{enrollment_type}_{suffix}.pkl"
        with open(output_path, "wb") as f:
            pickle.dump(gallery_embeddings, f)
        self.save_embeddings_json(gallery_embeddings, output_path)
        self._print(f"Saved to: {output_path}")
        return gallery_embeddings

    def _collect_enrollment(self, gallery_dir: Path) -> List[Tuple[str, List[Tuple[str, np.ndarray]]]]:
        """The file walk and one batched detect + align over all persons' files: per person (in sorted
        order) the (file name, first aligned face) of every file that gave a face."""
        person_dirs = sorted(d for d in gallery_dir.iterdir() if d.is_dir())
        listed = []
        for person_dir in person_dirs:
            image_files = _image_files(person_dir)
            if len(image_files) == 0:
                self._print(f"Warning: No images found for {person_dir.name}")
                continue
            listed.append((person_dir.name, image_files))
        results = iter(self._faces_of([str(p) for _person, files in listed for p in files]))
        persons = []
        for person_name, image_files in listed:
            kept = []
            for img_path in image_files:
                faces = next(results)
                if isinstance(faces, Exception):
                    self._print(f"Error processing {img_path}: {faces}")
                elif len(faces) == 0:
                    self._print(f"  No face detected in {img_path.name}")
                else:
                    kept.append((img_path.name, faces[0]["aligned_face"]))
            persons.append((person_name, kept))
        return persons

    def process_probe_positive(self, segmented: bool = False) -> Dict:
        self._print(f"\n{'=' * 60}")
        self._print(f"Processing Probe Positive: {'Segmented' if segmented else 'Unsegmented'}")
        self._print(f"{'=' * 60}\n")

        if segmented:
            probe_dir = self.output_root / "probe_labeled" / "segmented"
            categories = SEGMENT_CATEGORIES
        else:
            probe_dir = self.output_root / "probe_labeled" / "positive"
            categories = ["."]
        if not probe_dir.exists():
            self._print(f"Warning: Probe directory not found: {probe_dir}")
            return {}

        probe_embeddings = {}
        for category in categories:
            category_dir, category_name = (probe_dir, "all") if category == "." else (probe_dir / category, category)
            if not category_dir.exists():
                self._print(f"Warning: Category directory not found: {category_dir}")
                continue
            self._print(f"\nProcessing category: {category_name}")
            image_files = _image_files(category_dir)
            if len(image_files) == 0:
                self._print("  No images found")
                continue

            category_data = {}
            for img_path, embedding in self._embed_files(image_files):
                person_name = self.extract_name_from_filename(img_path.name)
                entry = category_data.setdefault(person_name, {"embeddings": [], "filenames": []})
                entry["embeddings"].append(embedding)
                entry["filenames"].append(img_path.name)
            for person_name in category_data:
                category_data[person_name]["embeddings"] = np.array(category_data[person_name]["embeddings"])
            probe_embeddings[category_name] = category_data
            self._print(f"  Processed {len(category_data)} persons, "
                        f"{sum(len(d['embeddings']) for d in category_data.values())} total images")

        suffix = "segmented" if segmented else "unsegmented"
        output_path = self.output_dir / f"probe_positive_{suffix}.pkl"
        with open(output_path, "wb") as f:
            pickle.dump(probe_embeddings, f)
        self.save_embeddings_json(probe_embeddings, output_path)
        self._print(f"\nSaved to: {output_path}")
        return probe_embeddings

    def process_probe_negative(self) -> Dict:
        self._print(f"\n{'=' * 60}")
        self._print("Processing Probe Negative")
        self._print(f"{'=' * 60}\n")

        probe_dir = self.output_root / "probe_labeled" / "negative"
        if not probe_dir.exists():
            self._print(f"Warning: Probe directory not found: {probe_dir}")
            return {}

        negative_embeddings = {"real": {"embeddings": [], "filenames": []},
                               "lfw": {"embeddings": [], "filenames": []}}
        image_files = _image_files(probe_dir)
        self._print(f"Found {len(image_files)} negative probe images")
        for img_path, embedding in self._embed_files(image_files):
            lfw = "lfw" in img_path.name.lower() or "lfw" in str(img_path.parent).lower()
            category = "lfw" if lfw else "real"
            negative_embeddings[category]["embeddings"].append(embedding)
            negative_embeddings[category]["filenames"].append(img_path.name)
        for category in negative_embeddings:
            if len(negative_embeddings[category]["embeddings"]) > 0:  # (an empty category keeps its list)
                negative_embeddings[category]["embeddings"] = np.array(negative_embeddings[category]["embeddings"])
                self._print(f"  {category}: {len(negative_embeddings[category]['embeddings'])} images")

        output_path = self.output_dir / "probe_negative.pkl"
        with open(output_path, "wb") as f:
            pickle.dump(negative_embeddings, f)
        self.save_embeddings_json(negative_embeddings, output_path)
        self._print(f"\nSaved to: {output_path}")
        return negative_embeddings

    def generate_all_embeddings(self):
        self._print(f"\n{'#' * 60}")
        self._print(f"# GENERATING ALL EMBEDDINGS - {self.model_name}")
        self._print(f"{'#' * 60}\n")

        start_time = datetime.now()
        self._crop_cache = {}
        try:
            self._print("\n[1/7] Gallery One-Shot BASE")
            gallery_oneshot_base = self.process_gallery_enrollment("one-shot", use_augmentation=False)
            self._print("\n[2/7] Gallery One-Shot AUGMENTED")
            gallery_oneshot_aug = self.process_gallery_enrollment("one-shot", use_augmentation=True)
            self._crop_cache.clear()
            self._print("\n[3/7] Gallery Few-Shot BASE")
            gallery_fewshot_base = self.process_gallery_enrollment("few-shot", use_augmentation=False)
            self._print("\n[4/7] Gallery Few-Shot AUGMENTED")
            gallery_fewshot_aug = self.process_gallery_enrollment("few-shot", use_augmentation=True)
        finally:
            self._crop_cache = None
        self._print("\n[5/7] Probe Positive (Unsegmented)")
        probe_positive_unseg = self.process_probe_positive(segmented=False)
        self._print("\n[6/7] Probe Positive (Segmented)")
        probe_positive_seg = self.process_probe_positive(segmented=True)
        self._print("\n[7/7] Probe Negative")
        probe_negative = self.process_probe_negative()
        duration = (datetime.now() - start_time).total_seconds()

        summary = {
            "model_type": self.model_type,
            "architecture": self.architecture,
            "model_name": self.model_name,
            "timestamp": datetime.now().isoformat(),
            "duration_seconds": duration,
            "gallery": {
                "one_shot_base_persons": len(gallery_oneshot_base),
                "one_shot_augmented_persons": len(gallery_oneshot_aug),
                "few_shot_base_persons": len(gallery_fewshot_base),
                "few_shot_augmented_persons": len(gallery_fewshot_aug),
            },
            "probe_positive": {
                "unsegmented_categories": list(probe_positive_unseg.keys()) if probe_positive_unseg else [],
                "segmented_categories": list(probe_positive_seg.keys()) if probe_positive_seg else [],
            },
            "probe_negative": {
                "real_images": len(probe_negative.get("real", {}).get("embeddings", [])),
                "lfw_images": len(probe_negative.get("lfw", {}).get("embeddings", [])),
            },
            "output_directory": str(self.output_dir),
        }
        summary_path = self.output_dir / "generation_summary.json"
        with open(summary_path, "w") as f:
            json.dump(summary, f, indent=2)
        self._print(f"\n{'=' * 60}")
        self._print("EMBEDDING GENERATION COMPLETE")
        self._print(f"{'=' * 60}")
        self._print(f"Model: {self.model_name}")
        self._print(f"Duration: {duration:.1f} seconds ({duration / 60:.1f} minutes)")
        self._print("\nGallery:")
        self._print(f"  One-shot base: {summary['gallery']['one_shot_base_persons']} persons")
        self._print(f"  One-shot augmented: {summary['gallery']['one_shot_augmented_persons']} persons")
        self._print(f"  Few-shot base: {summary['gallery']['few_shot_base_persons']} persons")
        self._print(f"  Few-shot augmented: {summary['gallery']['few_shot_augmented_persons']} persons")
        self._print("\nProbe Positive:")
        self._print(f"  Unsegmented categories: {len(summary['probe_positive']['unsegmented_categories'])}")
        self._print(f"  Segmented categories: {len(summary['probe_positive']['segmented_categories'])}")
        self._print("\nProbe Negative:")
        self._print(f"  Real images: {summary['probe_negative']['real_images']}")
        self._print(f"  LFW images: {summary['probe_negative']['lfw_images']}")
        self._print(f"\nOutput directory: {self.output_dir}")
        self._print(f"Summary saved to: {summary_path}")
        self._print(f"{'=' * 60}\n")


def build_parser() -> argparse.ArgumentParser:
    """The reference's command line (embedding_generator.py:435-464): same flags, defaults and choices."""
    parser = argparse.ArgumentParser(description="Generate face embeddings for evaluation using multiple models")
    parser.add_argument("--model_type", type=str, default="all", choices=["adaface", "arcface", "all"],
                        help="Model type to use (default: all models)")
    parser.add_argument("--architecture", type=str, default="all", choices=["ir_50", "ir_101", "all"],
                        help="Model architecture (default: all architectures)")
    parser.add_argument("--dataset_root", type=str, default=None,
                        help="Root directory for dataset (default: PROJECT_ROOT/dataset)")
    parser.add_argument("--output_root", type=str, default=None,
                        help="Root directory for outputs (default: PROJECT_ROOT/output/v0)")
    return parser


def main(argv=None, **injected):
    """The model x architecture loop of the reference's ``main``: a configuration that fails is
    printed with its traceback and the loop goes on.  ``injected``: keyword arguments for every
    ``EmbeddingGenerator`` built here (``face_processor=``, ``device=`` ...)."""
    args = build_parser().parse_args(argv)
    model_types = ["adaface", "arcface"] if args.model_type == "all" else [args.model_type]
    architectures = ["ir_50", "ir_101"] if args.architecture == "all" else [args.architecture]
    total_runs = len(model_types) * len(architectures)
    current_run = 0

    print(f"\n{'#' * 60}")
    print("# EMBEDDING GENERATION PIPELINE")
    print(f"# Total models to process: {total_runs}")
    print(f"{'#' * 60}\n")
    for model_type in model_types:
        for architecture in architectures:
            current_run += 1
            print(f"\n{'#' * 60}")
            print(f"# RUN {current_run}/{total_runs}")
            print(f"{'#' * 60}\n")
            try:
                generator = EmbeddingGenerator(model_type=model_type, architecture=architecture,
                                               dataset_root=args.dataset_root, output_root=args.output_root,
                                               **injected)
                generator.generate_all_embeddings()
            except Exception as e:
                print(f"\nERROR in {model_type}_{architecture}: {e}")
                import traceback
                traceback.print_exc()
                continue
    print(f"\n{'#' * 60}")
    print("# ALL EMBEDDING GENERATION COMPLETE")
    print(f"# Processed {total_runs} model configurations")
    print(f"{'#' * 60}\n")


if __name__ == "__main__":
    main()
