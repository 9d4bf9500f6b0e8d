"""Drop-in ``probe_labeler`` (probe_labeler.py): every crop of a probe folder is matched against a
gallery, labelled SURE / UNSURE / IMPOSTOR and copied under ``<name>_<file>`` -- the file names
``EmbeddingGenerator.extract_name_from_filename`` later reads the identity from.

Mirrors the reference class: ``determine_label``, ``match_face``, ``process_probe_directory`` and the
command line of ``main``, with the same arguments, return values, printed lines and
``labeling_results.json``.  The reference embeds and searches one file at a time; here the folder is
decoded in blocks of ``block_images`` files, each block embedded by one ``FaceEmbedder.embed_images``
call (crops of any mix of sizes) and matched by one ``GalleryManager.search_batch``.  Labels and
counts are made on the host from the floats ``search_batch`` returns.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
from datetime import datetime
from pathlib import Path
from typing import Dict, List, Optional, Tuple

import numpy as np

SCRIPT_DIR = Path(__file__).resolve().parent  # probe_labeler.py:14-17
IMAGE_SUFFIXES = (".jpg", ".jpeg", ".png", ".bmp")


class ProbeLabeler:
    def __init__(self, gallery_path=None, model_type="adaface", architecture="ir_101", sure_threshold=0.5,
                 unsure_threshold=0.4, *, embedder=None, gallery=None, device=None, verbose=True,
                 block_images: int = 1024):
        """The reference's arguments and defaults.  ``embedder`` and ``gallery`` inject existing objects
        instead of building the reference's defaults; ``device`` is the HIP device of the ones built
        here; ``block_images`` files are decoded, embedded and matched at a time."""
        if block_images < 1:
            raise ValueError("block_images must be at least 1")
        self.sure_threshold = sure_threshold
        self.unsure_threshold = unsure_threshold
        self.model_type = model_type
        self.architecture = architecture
        self.verbose = verbose
        self.block_images = int(block_images)
        if gallery_path is None:
            gallery_path = str(SCRIPT_DIR / "gallery" / "students.pkl")

        self._print("Initializing Probe Labeler...")
        self._print("=" * 70)
        self._print(f"Model: {model_type} - {architecture}")
        self._print(f"Sure threshold: {sure_threshold}")
        self._print(f"Unsure threshold: {unsure_threshold}")
        self._print("=" * 70)

        if embedder is None:
            from .face_embedder import FaceEmbedder
            embedder = FaceEmbedder(architecture=architecture, model_type=model_type, device=device)
        self.embedder = embedder
        if gallery is None:
            from .gallery_manager import GalleryManager
            gallery = GalleryManager(gallery_path=gallery_path, device=device, verbose=verbose)
        self.gallery = gallery

        num_students = len(self.gallery.get_all_students())
        if num_students == 0:
            self._print("\nWARNING: Gallery is empty! Please enroll students first.")
        else:
            self._print(f"   Loaded {num_students} enrolled students")
        self._print("\n" + "=" * 70)
        self._print("Probe Labeler ready!")
        self._print("=" * 70 + "\n")

    def _print(self, *args, **kw) -> None:
        if self.verbose:
            print(*args, **kw)

    def determine_label(self, confidence: float) -> str:
        if confidence >= self.sure_threshold:
            return "SURE"
        elif confidence >= self.unsure_threshold:
            return "UNSURE"
        else:
            return "IMPOSTOR"

    def _resolve(self, results) -> Tuple[Optional[str], str, float, str, List]:
        """probe_labeler.py:66-77 on one ``search`` result list."""
        if len(results) == 0:
            return None, "UNKNOWN", 0.0, "IMPOSTOR", []
        student_id, name, confidence = results[0]
        label = self.determine_label(confidence)
        top_matches = [{"student_id": sid, "name": n, "score": float(s), "rank": i + 1}
                       for i, (sid, n, s) in enumerate(results)]
        return student_id, name, float(confidence), label, top_matches

    def match_faces(self, face_images: List[np.ndarray], top_k: int = 3) -> List[Tuple]:
        """``match_face`` for a list of RGB crops of any sizes: one ``embed_images`` call and one
        ``search_batch``."""
        if len(face_images) == 0:
            return []
        if len(self.gallery.get_all_students()) == 0:  # search() of an empty gallery: no results
            return [self._resolve([]) for _ in face_images]
        emb = self.embedder.embed_images(face_images, normalize=True)
        emb = np.asarray(emb.cpu().numpy() if hasattr(emb, "cpu") else emb, dtype=np.float32)
        return [self._resolve(r) for r in self.gallery.search_batch(emb, top_k=top_k)]

    def match_face(self, face_image: np.ndarray, top_k: int = 3) -> Tuple[str, str, float, str, List]:
        return self.match_faces([face_image], top_k=top_k)[0]

    def process_probe_directory(self, probe_dir: str, output_dir: str = None, metadata_file: str = None,
                                copy_files: bool = True, top_k: int = 3) -> Dict:
        from .face_recognition import load_image_rgb
        if not os.path.exists(probe_dir):
            raise ValueError(f"Probe directory not found: {probe_dir}")
        if output_dir is None:
            output_dir = probe_dir + "_labeled"

        self._print("\n" + "=" * 70)
        self._print("LABELING PROBE FACES")
        self._print("=" * 70)
        self._print(f"Input directory: {probe_dir}")
        self._print(f"Output directory: {output_dir}")
        self._print("=" * 70 + "\n")

        os.makedirs(output_dir, exist_ok=True)
        label_dirs = {label: os.path.join(output_dir, label) for label in ("SURE", "UNSURE", "IMPOSTOR")}
        if copy_files:
            for d in label_dirs.values():
                os.makedirs(d, exist_ok=True)

        input_metadata = {}
        if metadata_file and os.path.exists(metadata_file):
            self._print(f"Loading metadata from: {metadata_file}")
            with open(metadata_file, "r") as f:
                for entry in json.load(f):
                    input_metadata[entry["filename"]] = entry
            self._print(f"Loaded metadata for {len(input_metadata)} images\n")

        image_files = sorted(f for f in os.listdir(probe_dir) if f.lower().endswith(IMAGE_SUFFIXES))
        if len(image_files) == 0:
            self._print("No image files found in probe directory!")
            return {"error": "no_images"}
        self._print(f"Found {len(image_files)} images to process\n")

        results = []
        label_counts = {"SURE": 0, "UNSURE": 0, "IMPOSTOR": 0}
        for at in range(0, len(image_files), self.block_images):
            block = image_files[at:at + self.block_images]
            images = [load_image_rgb(os.path.join(probe_dir, f)) for f in block]
            matched = iter(self.match_faces([im for im in images if im is not None], top_k=top_k))
            for idx, (image_file, image) in enumerate(zip(block, images), at + 1):
                image_path = os.path.join(probe_dir, image_file)
                self._print(f"[{idx}/{len(image_files)}] Processing: {image_file}")
                if image is None:
                    self._print("Failed to read image")
                    continue
                student_id, name, confidence, label, top_matches = next(matched)
                label_counts[label] += 1
                marker = "✓" if label == "SURE" else "⚠" if label == "UNSURE" else "✗"
                self._print(f"  {marker} {label}: {name} ({student_id}) - confidence: {confidence:.3f}")
                if len(top_matches) > 0:
                    self._print(f"     Top {len(top_matches)} matches:")
                    for match in top_matches:
                        self._print(f"       {match['rank']}. {match['name']} ({match['student_id']}): "
                                    f"{match['score']:.3f}")
                result = {
                    "filename": image_file,
                    "matched_student_id": student_id,
                    "matched_name": name,
                    "confidence": confidence,
                    "label": label,
                    "top_matches": top_matches,
                    "original_metadata": input_metadata.get(image_file, {}),
                }
                results.append(result)
                if copy_files:
                    dest_path = os.path.join(label_dirs[label], f"{name}_{image_file}")
                    shutil.copy2(image_path, dest_path)
                    result["labeled_path"] = dest_path

        summary = {
            "total_images": len(image_files),
            "processed": len(results),
            "label_distribution": label_counts,
            "sure_percentage": label_counts["SURE"] / len(results) * 100 if results else 0,
            "unsure_percentage": label_counts["UNSURE"] / len(results) * 100 if results else 0,
            "impostor_percentage": label_counts["IMPOSTOR"] / len(results) * 100 if results else 0,
            "settings": {
                "model_type": self.model_type,
                "architecture": self.architecture,
                "sure_threshold": self.sure_threshold,
                "unsure_threshold": self.unsure_threshold,
            },
            "timestamp": datetime.now().isoformat(),
        }
        results_file = os.path.join(output_dir, "labeling_results.json")
        with open(results_file, "w") as f:
            json.dump({"summary": summary, "results": results}, f, indent=2)
        self._print(f"\nResults saved to: {results_file}")
        self._print_summary(summary, output_dir if copy_files else None)
        return summary

    def _print_summary(self, summary: Dict, output_dir: str = None):
        self._print("\n" + "=" * 70)
        self._print("LABELING SUMMARY")
        self._print("=" * 70)
        self._print(f"Total images processed: {summary['processed']}/{summary['total_images']}")
        self._print("\nLabel Distribution:")
        self._print(f"  SURE:     {summary['label_distribution']['SURE']:3d} ({summary['sure_percentage']:.1f}%)")
        self._print(f"  UNSURE:   {summary['label_distribution']['UNSURE']:3d} ({summary['unsure_percentage']:.1f}%)")
        self._print(f"  IMPOSTOR: {summary['label_distribution']['IMPOSTOR']:3d} "
                    f"({summary['impostor_percentage']:.1f}%)")
        self._print("\nThresholds:")
        self._print(f"  Sure threshold:   ≥ {summary['settings']['sure_threshold']}")
        self._print(f"  Unsure threshold: ≥ {summary['settings']['unsure_threshold']}")
        if output_dir:
            self._print("\nLabeled images saved to:")
            for label in ("SURE", "UNSURE", "IMPOSTOR"):
                self._print(f"  {os.path.join(output_dir, label)}")
        self._print("=" * 70 + "\n")


def build_parser() -> argparse.ArgumentParser:
    """The reference's command line (probe_labeler.py:237-301): same flags, defaults and choices -- the
    command line's ``--unsure_threshold`` defaults to 0.3, the class's to 0.4, as there."""
    parser = argparse.ArgumentParser(description="Label probe faces by matching against gallery")
    parser.add_argument("--probe_dir", type=str, default=str(SCRIPT_DIR / "output" / "preprocessed" / "probe_positive"),
                        help="Directory containing probe face images")
    parser.add_argument("--output_dir", type=str, default=None, help='Output directory (default: probe_dir + "_labeled")')
    parser.add_argument("--metadata_file", type=str, default=None, help="Path to metadata JSON file from preprocessing")
    parser.add_argument("--gallery_path", type=str, default=str(SCRIPT_DIR / "gallery" / "students.pkl"),
                        help="Path to student gallery database")
    parser.add_argument("--model_type", type=str, default="adaface", choices=["adaface", "arcface"],
                        help="Type of face recognition model to use")
    parser.add_argument("--architecture", type=str, default="ir_101", choices=["ir_50", "ir_101"],
                        help="Model architecture")
    parser.add_argument("--sure_threshold", type=float, default=0.5, help="Confidence threshold for SURE label")
    parser.add_argument("--unsure_threshold", type=float, default=0.3,
                        help="Confidence threshold for UNSURE label (below = IMPOSTOR)")
    parser.add_argument("--top_k", type=int, default=3, help="Number of top matches to record")
    parser.add_argument("--no_copy", action="store_true", help="Do not copy files to labeled subdirectories")
    return parser


def main(argv=None, **injected):
    """``injected``: keyword arguments for the ``ProbeLabeler`` built here (``embedder=``, ``gallery=`` ...)."""
    args = build_parser().parse_args(argv)
    if args.metadata_file is None:
        potential_metadata = os.path.join(os.path.dirname(args.probe_dir), "probe_positive_metadata.json")
        if os.path.exists(potential_metadata):
            args.metadata_file = potential_metadata
    labeler = ProbeLabeler(gallery_path=args.gallery_path, model_type=args.model_type, architecture=args.architecture,
                           sure_threshold=args.sure_threshold, unsure_threshold=args.unsure_threshold, **injected)
    return labeler.process_probe_directory(probe_dir=args.probe_dir, output_dir=args.output_dir,
                                           metadata_file=args.metadata_file, copy_files=not args.no_copy,
                                           top_k=args.top_k)


if __name__ == "__main__":
    main()
