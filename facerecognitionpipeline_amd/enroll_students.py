"""Drop-in ``enroll_students`` (enroll_students.py:20-487): from a directory of photos to a
searchable, reference-readable gallery without leaving the library.

Mirrors the reference module -- ``augment_face_for_enrollment``, ``StudentEnrollment`` with
``process_student_directory`` / ``enroll_from_directory`` / ``verify_enrollment`` and the
command line of ``main`` -- with the same arguments, return dicts, error dicts, printed decisions
and exceptions.  What changes is where the work runs and how it is batched:

* the augmented copies of a face are made on the GPU (``fr_augment_faces``; cv2 is not needed);
* ``enroll_aligned`` takes the selected faces of MANY students, augments them in one launch per
  crop size, embeds all copies in ``max_batch`` chunks across student boundaries (the reference
  embeds 40 crops per student, one student at a time) and builds every template in one
  ``fr_build_templates`` launch (``GalleryManager.add_students_batch``);
* ``enroll_from_directory`` collects every student's faces first and then makes one
  ``enroll_aligned`` call; ``verify_enrollment`` is one ``search_batch``.

Only the first 14 entries of the reference's augmentation list exist here (enrollment uses 8):
entry 14 is ``cv2.GaussianBlur``, whose parity cannot be pinned without cv2, and entry 15 is
unseeded ``np.random.normal`` noise.  The rotations are pinned to this project's restatement of
OpenCV's fixed-point ``warpAffine`` (``oracle/align_ref.py``), not to cv2 itself (absent here).
"""
from __future__ import annotations

import argparse
import os
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib

PROJECT_ROOT = Path(__file__).resolve().parent.parent  # enroll_students.py:15-18

REFERENCE_AUGMENTATIONS = 16  # length of the reference's list (:22-46)
MAX_AUGMENTATIONS = 14        # FR_AUGMENT_MAX: the entries before GaussianBlur and noise
IMAGE_EXTENSIONS = {".jpg", ".jpeg", ".png", ".bmp"}


def _sliced_count(num_augmentations: int) -> int:
    """How many entries ``augmented[:num_augmentations]`` keeps of the reference's 16 (:48)."""
    return len(range(REFERENCE_AUGMENTATIONS)[:num_augmentations])


def _check_count(count: int) -> None:
    if count > MAX_AUGMENTATIONS:
        raise NotImplementedError(
            f"augmentations past the first {MAX_AUGMENTATIONS} are not implemented: entry 14 is cv2.GaussianBlur "
            "(parity cannot be pinned without cv2) and entry 15 is unseeded np.random.normal noise")


def augment_face_for_enrollment(face_image: np.ndarray, num_augmentations: int = 8, device=None) -> List[np.ndarray]:
    """enroll_students.py:20-48 for one HxWx3 uint8 crop, on the GPU: the crop, its mirror image,
    rotations by -10, -5, 5, 10 degrees (BORDER_REPLICATE), brightness -20, -10, 10, 20 and
    contrast 0.85, 0.92, 1.08, 1.15, cut to ``num_augmentations`` as the reference's slice cuts."""
    count = _sliced_count(num_augmentations)
    if count == 0:
        return []
    _check_count(count)
    img = np.asarray(face_image)
    if img.ndim != 3 or img.shape[2] != 3 or img.dtype != np.uint8:
        raise ValueError(f"expected an HxWx3 uint8 crop, got {img.dtype} {img.shape}")
    from .torch_ops import utility_handle
    h = utility_handle(device if device is not None else "cuda")
    crops = torch.from_numpy(np.ascontiguousarray(img)[None]).to(h.device)
    out = h.augment_faces(crops, count)[0].cpu().numpy()
    return [out[v] for v in range(count)]


def embed_augmented(embedder, handle: "_lib.Handle", device, faces: Sequence[np.ndarray],
                    augmentation_per_face: int) -> np.ndarray:
    """``augmentation_per_face`` copies of every crop of ``faces`` (HxWx3 uint8, any mix of sizes), made
    on ``handle`` and embedded by ``embedder`` with ``normalize=True`` -> host float32
    [len(faces) * A, 512], face-major and variant-minor.  One upload and one ``augment_faces`` launch per
    crop size; the forward runs in ``max_batch`` chunks.  (``StudentEnrollment`` and
    ``EmbeddingGenerator`` share it.)"""
    A = augmentation_per_face
    dev = torch.device(device)
    emb = torch.empty((len(faces), A, 512), dtype=torch.float32, device=dev)
    by_size: Dict[Tuple[int, int], List[int]] = {}
    for i, f in enumerate(faces):
        f = np.asarray(f)
        if f.ndim != 3 or f.shape[2] != 3 or f.dtype != np.uint8:
            raise ValueError(f"expected HxWx3 uint8 aligned crops, got {f.dtype} {f.shape}")
        by_size.setdefault(f.shape[:2], []).append(i)
    chunk = max(1, int(getattr(embedder, "max_batch", 256)))
    for (H, W), rows in by_size.items():
        crops = torch.from_numpy(np.ascontiguousarray(np.stack([np.asarray(faces[i]) for i in rows]))).to(dev)
        aug = handle.augment_faces(crops, A).reshape(len(rows) * A, H, W, 3)
        gemb = torch.empty((len(rows) * A, 512), dtype=torch.float32, device=dev)
        for off in range(0, len(aug), chunk):
            embedder.embed_tensor(aug[off:off + chunk], normalize=True, out=gemb[off:off + chunk])
        emb[torch.as_tensor(rows, device=dev)] = gemb.reshape(len(rows), A, 512)
    return emb.reshape(len(faces) * A, 512).cpu().numpy()


class StudentEnrollment:
    def __init__(self, gallery_path=PROJECT_ROOT / "gallery" / "students.pkl", min_faces_per_student=3,
                 max_faces_per_student=5, limit_images=0, image_indices=None, model_type="adaface",
                 architecture="ir_101", *, face_processor=None, embedder=None, gallery=None, device=None,
                 verbose=True):
        """The reference's arguments and defaults (:51-58).  ``face_processor``, ``embedder`` and
        ``gallery`` inject existing objects (sharing their handles) instead of building the
        reference's defaults; ``device`` is the HIP device of the ones built here."""
        self.min_faces = min_faces_per_student
        self.max_faces = max_faces_per_student
        self.limit_images = limit_images
        self.image_indices = image_indices
        self.verbose = verbose
        self.last_verification: Optional[Dict] = None

        self._print("Initializing enrollment system...")
        self._print("=" * 60)
        self._print("\n1. Loading face detection & alignment...")
        if face_processor is None:
            from .face_recognition import FaceProcessor
            face_processor = FaceProcessor(
                output_size=224, det_size=(640, 640), det_thresh=0.5,
                quality_filter_config={"min_det_score": 0.6, "min_face_size": 60, "max_yaw": 45, "max_pitch": 30,
                                       "max_roll": 30, "check_blur": True, "blur_threshold": 100},
                providers=["CUDAExecutionProvider", "CPUExecutionProvider"], device=device)
        self.face_processor = face_processor

        self._print("\n2. Loading AdaFace model...")
        if embedder is None:
            from .face_embedder import FaceEmbedder
            embedder = FaceEmbedder(architecture=architecture, model_type=model_type, device=device)
        self.embedder = embedder

        self._print("\n3. Loading gallery database...")
        if gallery is None:
            from .gallery_manager import GalleryManager
            gallery = GalleryManager(gallery_path=str(gallery_path), aggregation_method="weighted_mean",
                                     device=device, verbose=verbose)
        self.gallery = gallery
        self._device = torch.device(device) if device is not None else None

        self._print("\n" + "=" * 60)
        self._print("Enrollment system ready!")
        self._print("=" * 60 + "\n")

    def _print(self, *args, **kw) -> None:
        if self.verbose:
            print(*args, **kw)

    # -- reference API -------------------------------------------------------
    def _deduplicate_embeddings(self, embeddings: np.ndarray, threshold: float = 0.95) -> np.ndarray:
        """enroll_students.py:99-117 (unused by the flow there as here; kept for API parity):
        greedily drop every later embedding whose dot product with a kept one exceeds
        ``threshold``."""
        if len(embeddings) <= 1:
            return embeddings
        keep = np.ones(len(embeddings), dtype=bool)
        for i in range(len(embeddings)):
            if not keep[i]:
                continue
            dup = np.where(np.dot(embeddings[i:], embeddings[i]) > threshold)[0]
            if len(dup) > 1:
                keep[i + dup[1:]] = False
        kept = embeddings[keep]
        self._print(f"  Deduplication: kept {len(kept)}/{len(embeddings)} unique embeddings")
        return kept

    # -- the device path -----------------------------------------------------
    @property
    def device(self) -> torch.device:
        dev = getattr(self.embedder, "device", None) or self._device
        if dev is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        return torch.device(dev)

    def _ops_handle(self) -> "_lib.Handle":
        """The handle the augmentation runs on: the embedder's own (same device, same stream
        order as the forward that follows) or the device's model-less utility handle."""
        model = getattr(self.embedder, "model", None)
        if isinstance(model, _lib.Handle):
            return model
        from .torch_ops import utility_handle
        return utility_handle(self.device)

    def _embed_augmented(self, faces: Sequence[np.ndarray], augmentation_per_face: int) -> np.ndarray:
        """``augmentation_per_face`` copies of every crop of ``faces`` (HxWx3 uint8, any mix of
        sizes), embedded with ``normalize=True`` -> host float32 [len(faces) * A, 512], face-major
        and variant-minor (the reference's ``all_face_images`` order, :212-222).  One upload and
        one ``augment_faces`` launch per crop size; the forward runs in ``max_batch`` chunks."""
        return embed_augmented(self.embedder, self._ops_handle(), self.device, faces, augmentation_per_face)

    def enroll_aligned(self, students: Sequence[Tuple], augmentation_per_face: int = 8) -> List[Tuple[bool, Dict]]:
        """Enroll many students from their aligned crops in one pass.  ``students``: (student_id,
        name, [HxWx3 uint8 crops], metadata_extra) -- ``metadata_extra`` (or None) may give the
        record's ``num_images`` and ``source_directory``.  Per student, what
        ``process_student_directory`` does from :208 on: augmentation, embeddings, the intra-class
        similarity (and its warning), ``add_student(..., overwrite=True)`` with the six metadata
        keys of :239-246 -- but with all crops augmented and embedded together and all templates
        built by one ``add_students_batch``.  Returns (success, info) per student, info as
        :253-260; a student without crops fails with the ``insufficient_faces`` dict."""
        A = _sliced_count(augmentation_per_face)
        _check_count(A)
        if A < 1:
            raise ValueError("augmentation_per_face must keep at least one copy per face")
        students = [(s[0], s[1], list(s[2]), (s[3] if len(s) > 3 else None) or {}) for s in students]
        faces = [f for _sid, _name, crops, _extra in students for f in crops]
        allemb = self._embed_augmented(faces, A) if faces else np.zeros((0, 512), np.float32)
        results: List[Optional[Tuple[bool, Dict]]] = []
        entries, enrolled = [], []
        row = 0
        for i, (sid, name, crops, extra) in enumerate(students):
            if not crops:
                results.append((False, {"error": "insufficient_faces", "valid_faces": 0, "required": self.min_faces}))
                continue
            n_aug = len(crops) * A
            self._print(f"\n  Applying augmentation to {len(crops)} faces...")
            self._print(f"  Generated {n_aug} augmented faces ({A} per original)")
            self._print("  Extracting embeddings...")
            embeddings = np.ascontiguousarray(allemb[row:row + n_aug])
            row += n_aug
            self._print(f"  Extracted {len(embeddings)} embeddings (512-dim)")
            # the reference's own expression (:227-228), float32 as there
            similarities = np.dot(embeddings, embeddings.T)
            avg_similarity = (np.sum(similarities) - len(embeddings)) / (len(embeddings) * (len(embeddings) - 1))
            self._print(f"  Average intra-class similarity: {avg_similarity:.4f}")
            if avg_similarity < 0.3:
                self._print(f"\nWarning: Low intra-class similarity ({avg_similarity:.4f})")
                self._print("   Images may contain different people or very different poses")
            num_images = extra.get("num_images", len(crops))
            metadata = {"num_images": num_images, "num_valid_faces": len(crops), "num_augmented_faces": n_aug,
                        "augmentation_per_face": A, "avg_similarity": float(avg_similarity),
                        "source_directory": extra.get("source_directory")}
            entries.append((sid, name, embeddings, metadata))
            enrolled.append(i)
            results.append((True, {"student_id": sid, "name": name, "num_images": num_images,
                                   "num_valid_faces": len(crops), "num_embeddings": len(embeddings),
                                   "avg_similarity": float(avg_similarity)}))
        if entries:
            self.gallery.add_students_batch(entries, overwrite=True)
            for i in enrolled:
                self._print(f"\nSuccessfully enrolled {students[i][1]} ({students[i][0]})")
        return results

    def _next_default_id(self, taken: set) -> str:
        return f"STU{len(taken) + 1:04d}"

    def _collect_student(self, student_dir: str, student_id: Optional[str], taken: set):
        """enroll_students.py:122-206: the file walk, the image selection, detection + alignment,
        the best face per image and the min / max face selection.  ``taken``: the ids the gallery
        holds once the students collected so far are enrolled, so a default id is what the
        reference's one-by-one loop gives (:123-125).  Returns (entry for ``enroll_aligned``,
        None) or (None, error dict)."""
        student_name = os.path.basename(student_dir)
        if student_id is None:
            student_id = self._next_default_id(taken)

        self._print(f"\n{'=' * 60}")
        self._print(f"Processing: {student_name}")
        self._print(f"Student ID: {student_id}")
        self._print(f"{'=' * 60}")

        image_files = sorted(os.path.join(student_dir, f) for f in sorted(os.listdir(student_dir))
                             if os.path.splitext(f)[1].lower() in IMAGE_EXTENSIONS)
        if len(image_files) == 0:
            self._print(f"No images found in {student_dir}")
            return None, {"error": "no_images"}

        if self.image_indices:
            selected = []
            for idx in self.image_indices:
                if 1 <= idx <= len(image_files):
                    selected.append(image_files[idx - 1])
                else:
                    self._print(f"Warning: image index {idx} out of range (1-{len(image_files)})")
            image_files = selected
            self._print(f"Using explicit image indices: {self.image_indices}")
        elif self.limit_images > 0:
            image_files = image_files[:self.limit_images]
            self._print(f"Limiting to first {self.limit_images} images")

        self._print(f"Found {len(image_files)} images")
        all_faces, valid_faces = [], []
        for idx, img_path in enumerate(image_files, 1):
            self._print(f"\n  [{idx}/{len(image_files)}] Processing {os.path.basename(img_path)}...", end=" ")
            try:
                faces = self.face_processor.process_image(img_path, return_all=True)
                if len(faces) == 0:
                    self._print("No faces detected")
                    continue
                best_face = faces[0]
                all_faces.append(best_face)
                if best_face["is_valid"]:
                    valid_faces.append(best_face)
                    quality = best_face["quality_metrics"]
                    self._print(f"✓ Valid face (score: {best_face['det_score']:.3f}, "
                                f"blur: {quality.get('blur_score', 0):.0f})")
                else:
                    self._print("Low quality face")
            except Exception as e:  # as the reference: a bad image is reported and skipped (:186-188)
                self._print(f"Error: {e}")
                continue

        self._print(f"\n  Summary: {len(valid_faces)}/{len(all_faces)} valid faces")
        if len(valid_faces) < self.min_faces:
            self._print(f"\nInsufficient valid faces ({len(valid_faces)} < {self.min_faces})")
            self._print(f"   Please provide more high-quality images for {student_name}")
            return None, {"error": "insufficient_faces", "valid_faces": len(valid_faces), "required": self.min_faces}

        if len(valid_faces) > self.max_faces:
            self._print(f"  Using top {self.max_faces} faces (sorted by quality)")
            valid_faces.sort(key=lambda x: x["det_score"] * x["quality_metrics"].get("blur_score", 1000),
                             reverse=True)
            valid_faces = valid_faces[:self.max_faces]

        taken.add(student_id)
        extra = {"num_images": len(image_files), "source_directory": student_dir}
        return (student_id, student_name, [f["aligned_face"] for f in valid_faces], extra), None

    def _gallery_ids(self) -> set:
        return set(self.gallery.get_all_students().keys())

    def process_student_directory(self, student_dir: str, student_id: str = None) -> Tuple[bool, Dict]:
        """enroll_students.py:119-260 for one student directory."""
        entry, error = self._collect_student(student_dir, student_id, self._gallery_ids())
        if entry is None:
            return False, error
        return self.enroll_aligned([entry])[0]

    def enroll_from_directory(self, enrollment_dir: str) -> Dict:
        """enroll_students.py:262-346: every sub-directory is one student.  All students' faces are
        collected first and enrolled by one ``enroll_aligned`` call."""
        if not os.path.exists(enrollment_dir):
            raise ValueError(f"Enrollment directory not found: {enrollment_dir}")

        self._print("\n" + "=" * 60)
        self._print(f"ENROLLMENT FROM: {enrollment_dir}")
        self._print("=" * 60)

        student_dirs = [p for p in (os.path.join(enrollment_dir, item) for item in sorted(os.listdir(enrollment_dir)))
                        if os.path.isdir(p)]
        if len(student_dirs) == 0:
            self._print("No student directories found!")
            return {"error": "no_directories"}
        self._print(f"Found {len(student_dirs)} student directories")

        taken = self._gallery_ids()
        collected = [self._collect_student(d, None, taken) for d in student_dirs]
        entries = [entry for entry, _error in collected if entry is not None]
        enrolled = iter(self.enroll_aligned(entries) if entries else [])

        results = []
        successful = failed = 0
        for student_dir, (entry, error) in zip(student_dirs, collected):
            success, info = next(enrolled) if entry is not None else (False, error)
            if success:
                successful += 1
            else:
                failed += 1
            results.append({"directory": student_dir, "success": success, "info": info})

        self._print("\n" + "=" * 60)
        self._print("Saving gallery...")
        self.gallery.save()

        self._print("\n" + "=" * 60)
        self._print("ENROLLMENT SUMMARY")
        self._print("=" * 60)
        self._print(f"Total students processed: {len(student_dirs)}")
        self._print(f"Successfully enrolled: {successful}")
        self._print(f"Failed: {failed}")

        if successful > 0:
            self._print("\nEnrolled students:")
            for result in results:
                if result["success"]:
                    info = result["info"]
                    self._print(f"  • {info['name']} ({info['student_id']}): "
                                f"{info['num_embeddings']} embeddings "
                                f"(from {info.get('num_valid_faces', '?')} faces) "
                                f"(similarity: {info['avg_similarity']:.3f})")
        if failed > 0:
            self._print("\nFailed enrollments:")
            for result in results:
                if not result["success"]:
                    name = os.path.basename(result["directory"])
                    self._print(f"  • {name}: {result['info'].get('error', 'unknown')}")

        stats = self.gallery.get_statistics()
        self._print("\nGallery statistics:")
        self._print(f"  Total students: {stats['num_students']}")
        self._print(f"  Total embeddings: {stats['total_embeddings']}")
        self._print(f"  Avg per student: {stats['avg_embeddings_per_student']:.1f}")
        self._print("\n" + "=" * 60)

        if successful > 0:
            self.verify_enrollment()

        return {"total": len(student_dirs), "successful": successful, "failed": failed, "results": results,
                "gallery_stats": stats}

    def verify_enrollment(self):
        """enroll_students.py:350-402: every student's first embedding must find that student at
        rank 1; one ``search_batch`` (top 3) instead of a search per student.  Returns None like
        the reference; the figures are kept in ``self.last_verification``."""
        self._print("\n" + "=" * 60)
        self._print("ENROLLMENT VERIFICATION")
        self._print("=" * 60)

        self.last_verification = None
        students = self.gallery.get_all_students()
        if len(students) < 2:
            self._print("Need at least 2 students for verification")
            return

        self._print(f"\nTesting {len(students)} enrolled students...")
        records = list(students.values())
        queries = np.stack([np.asarray(r.embeddings[0], np.float32) for r in records])
        all_results = self.gallery.search_batch(queries, top_k=3)

        correct_matches = 0
        total_tests = 0
        inter_class_sims = []
        for student, results in zip(records, all_results):
            _top_id, top_name, top_score = results[0]
            if top_name == student.name:
                correct_matches += 1
            else:
                self._print(f"  ✗ Invalid {student.name}: Matched to {top_name} (score: {top_score:.3f})")
            total_tests += 1
            inter_class_sims.extend(score for _id, _name, score in results[1:])

        accuracy = correct_matches / total_tests * 100
        avg_inter_class = np.mean(inter_class_sims) if inter_class_sims else 0
        max_inter_class = np.max(inter_class_sims) if inter_class_sims else 0
        self.last_verification = {"correct": correct_matches, "total": total_tests, "accuracy": accuracy,
                                  "avg_inter_class": float(avg_inter_class),
                                  "max_inter_class": float(max_inter_class)}

        self._print("\nVerification Results:")
        self._print(f"  Rank-1 Accuracy: {correct_matches}/{total_tests} ({accuracy:.1f}%)")
        self._print(f"  Avg inter-class similarity: {avg_inter_class:.3f}")
        self._print(f"  Max inter-class similarity: {max_inter_class:.3f}")
        if accuracy < 100:
            self._print(f"\nWarning: {total_tests - correct_matches} student(s) failed verification!")
            self._print("   Check if images contain the correct person")
        if max_inter_class > 0.6:
            self._print(f"\nWarning: High inter-class similarity detected ({max_inter_class:.3f})")
            self._print("   Some students may look very similar or be duplicates")
        if accuracy == 100 and max_inter_class < 0.5:
            self._print("\nAll students verified successfully!")
        self._print("=" * 60)


def build_parser() -> argparse.ArgumentParser:
    """The reference's command line (enroll_students.py:405-461): same flags, defaults and choices."""
    parser = argparse.ArgumentParser(description="Enroll students from directory structure")
    parser.add_argument("--enrollment_dir", type=str, default=str(PROJECT_ROOT / "samples" / "enrollment"),
                        help="Directory containing student subdirectories")
    parser.add_argument("--gallery_path", type=str, default=str(PROJECT_ROOT / "gallery" / "students.pkl"),
                        help="Path to gallery database")
    parser.add_argument("--min_faces", type=int, default=1, help="Minimum valid faces required per student")
    parser.add_argument("--max_faces", type=int, default=5, help="Maximum faces to use per student")
    parser.add_argument("--limit_images", type=int, default=0,
                        help="Limit how many images per student to process (0 = all)")
    parser.add_argument("--image_indices", type=int, nargs="*", default=None,
                        help="Explicit list of image numbers to use (1-based). Example: 2 3 4")
    parser.add_argument("--model_type", type=str, default="adaface", choices=["adaface", "arcface"],
                        help="Type of face recognition model to use")
    parser.add_argument("--architecture", type=str, default="ir_101", choices=["ir_50", "ir_101"],
                        help="Model architecture (ir_50 or ir_101)")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    enrollment = StudentEnrollment(gallery_path=args.gallery_path, min_faces_per_student=args.min_faces,
                                   max_faces_per_student=args.max_faces, limit_images=args.limit_images,
                                   image_indices=args.image_indices, model_type=args.model_type,
                                   architecture=args.architecture)
    summary = enrollment.enroll_from_directory(args.enrollment_dir)
    if summary.get("successful", 0) > 0:
        print("\nCreating backup...")
        backup_dir = PROJECT_ROOT / "gallery" / "backups"
        enrollment.gallery.export_for_backup(str(backup_dir), backup_name=f"{args.model_type}_{args.architecture}")
        print(f"Backup saved to {backup_dir}")


if __name__ == "__main__":
    main()
