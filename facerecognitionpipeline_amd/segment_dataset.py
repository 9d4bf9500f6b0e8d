"""Drop-in ``ProbeSegmenter`` (segment_dataset.py): bucket the aligned probe crops that
``DatasetPreprocessor`` wrote by pose, face size, blur and detection score.

Pure host code over the metadata list: every decision is the reference module's, quirks included
(``tests/golden/segment_dataset.npz`` pins thresholds, categories and the written metadata):

* the two blur thresholds are order statistics of the data set's own blur scores, index
  ``int(len * (1 - sharp_percentile / 100))`` and ``int(len * blurry_percentile / 100)``; an index at
  ``len`` gives threshold 0;
* a face can be ``blur_sharp`` and ``blur_blurry`` at once (both tests are inclusive);
* ``baseline`` compares the detection score with the literal 0.7, whatever ``det_score_threshold`` is;
* a metadata entry is matched to the first listed file whose name *ends with* its ``filename``
  (``os.listdir`` order in the reference; sorted here, so the choice among several is deterministic).

The buckets are the ones ``evaluate_models.evaluate_segmented_comprehensive`` reads.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
from typing import Dict, List

CATEGORIES = ["baseline", "pose_easy", "pose_medium", "pose_hard", "face_large", "face_medium", "face_small",
              "blur_sharp", "blur_blurry", "low_quality"]
BASELINE_DET_SCORE = 0.7  # the reference's literal, not det_score_threshold


class ProbeSegmenter:
    def __init__(self, pose_easy_threshold: float = 15.0, pose_medium_threshold: float = 30.0,
                 face_large_threshold: int = 150, face_medium_threshold: int = 80,
                 blur_sharp_percentile: float = 50.0, blur_blurry_percentile: float = 20.0,
                 det_score_threshold: float = 0.7, verbose: bool = True):
        self.pose_easy_threshold = pose_easy_threshold
        self.pose_medium_threshold = pose_medium_threshold
        self.face_large_threshold = face_large_threshold
        self.face_medium_threshold = face_medium_threshold
        self.blur_sharp_percentile = blur_sharp_percentile
        self.blur_blurry_percentile = blur_blurry_percentile
        self.det_score_threshold = det_score_threshold
        self.blur_sharp_threshold = None
        self.blur_blurry_threshold = None
        self.categories = list(CATEGORIES)
        self.verbose = verbose

    def _say(self, *a) -> None:
        if self.verbose:
            print(*a)

    def compute_blur_thresholds(self, metadata_list: List[Dict]) -> None:
        scores = sorted(m.get("blur_score", 0.0) for m in metadata_list)
        n = len(scores)
        sharp = int(n * (1 - self.blur_sharp_percentile / 100.0))
        blurry = int(n * (self.blur_blurry_percentile / 100.0))
        self.blur_sharp_threshold = scores[sharp] if sharp < n else 0
        self.blur_blurry_threshold = scores[blurry] if blurry < n else 0
        self._say(f"  Blur sharp threshold: {self.blur_sharp_threshold:.2f}")
        self._say(f"  Blur blurry threshold: {self.blur_blurry_threshold:.2f}")

    @staticmethod
    def _pose_angle(metadata: Dict) -> float:
        return (abs(metadata.get("yaw", 0.0)) ** 2 + abs(metadata.get("pitch", 0.0)) ** 2) ** 0.5

    def categorize_face(self, metadata: Dict) -> List[str]:
        pose = self._pose_angle(metadata)
        blur = metadata.get("blur_score", 0.0)
        det = metadata.get("det_score", 1.0)
        size = metadata.get("face_size", 0)
        out = []
        if (pose <= self.pose_easy_threshold and size >= self.face_medium_threshold
                and blur >= self.blur_sharp_threshold and det >= BASELINE_DET_SCORE):
            out.append("baseline")
        out.append("pose_easy" if pose <= self.pose_easy_threshold else
                   "pose_medium" if pose <= self.pose_medium_threshold else "pose_hard")
        out.append("face_large" if size >= self.face_large_threshold else
                   "face_medium" if size >= self.face_medium_threshold else "face_small")
        if blur >= self.blur_sharp_threshold:
            out.append("blur_sharp")
        if blur <= self.blur_blurry_threshold:
            out.append("blur_blurry")
        if det < self.det_score_threshold:
            out.append("low_quality")
        return out

    def build_filename_mapping(self, input_dir: str, metadata_list: List[Dict]) -> Dict[str, str]:
        files = sorted(os.listdir(input_dir))
        mapping: Dict[str, str] = {}
        missing = []
        for m in metadata_list:
            name = m["filename"]
            hit = next((f for f in files if f.endswith(name)), None)
            if hit is None:
                missing.append(name)
            else:
                mapping[name] = hit
        if missing:
            self._say(f"\nWarning: {len(missing)} metadata entries without matching files:")
            for name in missing[:10]:
                self._say(f"  - {name}")
            if len(missing) > 10:
                self._say(f"  ... and {len(missing) - 10} more")
        self._say(f"\nSuccessfully mapped {len(mapping)}/{len(metadata_list)} files")
        return mapping

    def segment_dataset(self, input_dir: str, metadata_file: str, output_dir: str, copy_files: bool = True) -> None:
        with open(metadata_file, "r") as f:
            metadata_list = json.load(f)
        self._say(f"Loaded metadata for {len(metadata_list)} faces from {metadata_file}")
        self.compute_blur_thresholds(metadata_list)
        mapping = self.build_filename_mapping(input_dir, metadata_list)
        dirs = {}
        for c in self.categories:
            dirs[c] = os.path.join(output_dir, c)
            os.makedirs(dirs[c], exist_ok=True)
        counts = {c: 0 for c in self.categories}
        processed = skipped = 0
        for m in metadata_list:
            actual = mapping.get(m["filename"])
            src = None if actual is None else os.path.join(input_dir, actual)
            if src is None or not os.path.exists(src):
                self._say(f"Warning: no file for metadata entry {m['filename']}")
                skipped += 1
                continue
            for c in self.categorize_face(m):
                dst = os.path.join(dirs[c], actual)
                try:
                    if copy_files:
                        shutil.copy2(src, dst)
                    else:
                        if os.path.exists(dst):
                            os.remove(dst)
                        os.symlink(os.path.relpath(src, dirs[c]), dst)
                    counts[c] += 1
                except Exception as e:  # the reference reports and goes on
                    self._say(f"Error processing {actual} -> {c}: {e}")
            processed += 1
        # every entry of a category goes into its metadata, with or without a file
        for c in self.categories:
            rows = []
            for m in metadata_list:
                if c in self.categorize_face(m):
                    row = dict(m)
                    if m["filename"] in mapping:
                        row["labeled_filename"] = mapping[m["filename"]]
                    rows.append(row)
            with open(os.path.join(dirs[c], f"{c}_metadata.json"), "w") as f:
                json.dump(rows, f, indent=2)
        self._say(f"Total faces processed: {processed}; skipped (not found): {skipped}")
        for c in self.categories:
            share = counts[c] / processed * 100 if processed else 0
            self._say(f"  {c:15s}: {counts[c]:5d} faces ({share:5.1f}%)")
        self.print_quality_insights(metadata_list)

    def print_quality_insights(self, metadata_list: List[Dict]) -> None:
        """The reference's report: how many entries each test of ``categorize_face`` puts in each bucket,
        as counts and shares of the list (an empty list divides by zero, as there)."""
        cats = [self.categorize_face(m) for m in metadata_list]
        total = len(metadata_list)

        def line(label: str, category: str) -> str:
            n = sum(category in c for c in cats)
            return f"{label}: {n}/{total} ({n / total * 100:.1f}%)"

        print("Quality Insights:")
        print("-" * 70)
        print("  " + line("Baseline (clean) faces", "baseline"))
        print("\n  Pose Distribution:")
        for label, c in (("Easy", "pose_easy"), ("Medium", "pose_medium"), ("Hard", "pose_hard")):
            print("    " + line(label, c))
        print("\n  Face Size Distribution:")
        for label, c in (("Large", "face_large"), ("Medium", "face_medium"), ("Small", "face_small")):
            print("    " + line(label, c))
        print("\n  Blur Distribution:")
        for label, c in (("Sharp", "blur_sharp"), ("Blurry", "blur_blurry")):
            print("    " + line(label, c))
        print("\n  " + line("Low detection score", "low_quality"))
        print("=" * 70 + "\n")


def build_parser() -> argparse.ArgumentParser:
    """The reference's command line (segment_dataset.py): same flags and defaults.  ``--yaw_threshold``,
    ``--pitch_threshold`` and ``--blur_threshold`` are accepted and unused, as there."""
    p = argparse.ArgumentParser(description="Segment probe dataset based on quality metrics for evaluation")
    p.add_argument("--input_dir", type=str, default="output/preprocessed/probe_positive",
                   help="Directory containing probe images")
    p.add_argument("--metadata_file", type=str, default="output/preprocessed/probe_positive_metadata.json",
                   help="Path to metadata JSON file")
    p.add_argument("--output_dir", type=str, default="output/preprocessed/segmented",
                   help="Output directory for segmented images")
    p.add_argument("--yaw_threshold", type=float, default=35.0, help="Unused (kept for the reference's command line)")
    p.add_argument("--pitch_threshold", type=float, default=25.0, help="Unused (kept for the reference's command line)")
    p.add_argument("--blur_threshold", type=float, default=50.0, help="Unused (kept for the reference's command line)")
    p.add_argument("--symlink", action="store_true", help="Create symlinks instead of copying files")
    p.add_argument("--pose_easy_threshold", type=float, default=15.0, help="Pose angle limit of pose_easy (degrees)")
    p.add_argument("--pose_medium_threshold", type=float, default=30.0,
                   help="Pose angle limit of pose_medium (degrees)")
    p.add_argument("--face_large_threshold", type=int, default=150, help="Face size from which a face is large (px)")
    p.add_argument("--face_medium_threshold", type=int, default=80, help="Face size from which a face is medium (px)")
    p.add_argument("--blur_sharp_percentile", type=float, default=50.0, help="Top percentile that counts as sharp")
    p.add_argument("--blur_blurry_percentile", type=float, default=20.0,
                   help="Bottom percentile that counts as blurry")
    p.add_argument("--det_score_threshold", type=float, default=0.7,
                   help="Detection score below which a face is low_quality")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    segmenter = ProbeSegmenter(pose_easy_threshold=args.pose_easy_threshold,
                               pose_medium_threshold=args.pose_medium_threshold,
                               face_large_threshold=args.face_large_threshold,
                               face_medium_threshold=args.face_medium_threshold,
                               blur_sharp_percentile=args.blur_sharp_percentile,
                               blur_blurry_percentile=args.blur_blurry_percentile,
                               det_score_threshold=args.det_score_threshold)
    segmenter.segment_dataset(input_dir=args.input_dir, metadata_file=args.metadata_file,
                              output_dir=args.output_dir, copy_files=not args.symlink)


if __name__ == "__main__":
    main()
