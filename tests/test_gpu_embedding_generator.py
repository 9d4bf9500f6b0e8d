"""``EmbeddingGenerator`` and ``ProbeLabeler`` on the GPU against what the REFERENCE classes computed with
the reference ``FaceEmbedder`` on the same synthetic ``ir_50`` weights
(``tests/golden/embedding_tools.npz``, ``real__*``; recorded by tools/make_golden_embeddings.py): every
embedding within 1e-5, structures, keys, file names and JSON key sets equal; the written files feed
``load_all_embeddings`` and the evaluation; the labeler with the real ``GalleryManager`` reproduces the
reference's labels, counts, copied names and top-k ids, scores within 1e-5.  (Confidences that sit
exactly on a threshold are checked on the host, tests/test_embedding_tools.py: the GPU's fp32 dot
need not land on the same float.)
"""
import json
import os
import pickle

import numpy as np
import pytest

from tests import _embedding_cases as EC

pytestmark = pytest.mark.gpu

EMB_TOL = 1e-5
SCORE_TOL = 1e-5


@pytest.fixture(scope="module")
def golden(golden_dir):
    g = np.load(os.path.join(golden_dir, "embedding_tools.npz"))
    assert str(g["trees_sha256"]) == EC.trees_sha256()
    return g


@pytest.fixture(scope="module")
def emb():
    from facerecognitionpipeline_amd.face_embedder import FaceEmbedder
    return FaceEmbedder(architecture=EC.ARCHITECTURE, model_path="synthetic", max_batch=16)


@pytest.fixture(scope="module")
def generated(emb, tmp_path_factory):
    from facerecognitionpipeline_amd.embedding_generator import EmbeddingGenerator
    root = tmp_path_factory.mktemp("gpu_embedding_tools")
    dataset = EC.build_dataset(str(root / "dataset"))
    output = EC.build_probes(str(root / "output"))
    g = EmbeddingGenerator(EC.MODEL_TYPE, EC.ARCHITECTURE, dataset_root=dataset, output_root=output,
                           face_processor=EC.BatchStubProcessor(), embedder=emb, verbose=False, block_images=3)
    g.generate_all_embeddings()
    return g


def _key_sets(doc):
    if isinstance(doc, dict):
        return {k: _key_sets(v) for k, v in doc.items()}
    if isinstance(doc, list):
        return ["list", len(doc)] if not doc or not isinstance(doc[0], (dict, list)) else ["rows", len(doc), len(doc[0])]
    return type(doc).__name__


def test_generated_files_match_the_reference(golden, generated):
    out = str(generated.output_dir)
    files = sorted(os.path.relpath(os.path.join(d, f), out) for d, _s, fs in os.walk(out) for f in fs)
    assert files == json.loads(str(golden["real__files"]))
    structs, keys = json.loads(str(golden["real__structs"])), json.loads(str(golden["real__json_keys"]))
    arrays = {}
    for stem in EC.EMBEDDING_OUTPUTS:
        with open(os.path.join(out, stem + ".pkl"), "rb") as f:
            assert EC.pack(pickle.load(f), arrays, stem) == structs[stem], stem
        with open(os.path.join(out, stem + ".json")) as f:
            assert _key_sets(json.load(f)) == keys[stem], stem
    worst = 0.0
    for k, v in arrays.items():
        worst = max(worst, float(np.abs(v - golden[f"real__{k}"]).max()))
    print("EmbeddingGenerator vs the reference: max abs embedding difference", worst, "over", len(arrays), "arrays")
    assert len(arrays) >= 20 and worst <= EMB_TOL
    with open(os.path.join(out, "generation_summary.json")) as f:
        assert EC.strip_summary(json.load(f)) == json.loads(str(golden["real__summary"]))
    assert generated.face_processor.calls == [5, 7]


def test_written_files_feed_the_evaluation(generated, emb):
    from facerecognitionpipeline_amd import evaluate_models as EM
    loaded = EM.load_all_embeddings(generated.output_root / "embeddings")[EC.MODEL_NAME]
    assert set(loaded) == set(EM.EMBEDDING_FILES)
    res = EM.evaluate_probes_comprehensive(loaded["gallery_fewshot_augmented"], loaded["probe_positive_unsegmented"],
                                           [0.3, 0.5], aggregation="max", device=emb.device)
    assert len(res["all_predictions"]) == 7  # the decodable, listed files of probe_labeled/positive
    assert 0.0 <= float(res["threshold_results"][0]["rank1_accuracy"]) <= 1.0


def test_labeler_matches_the_reference(golden, emb, tmp_path):
    from facerecognitionpipeline_amd.gallery_manager import GalleryManager
    from facerecognitionpipeline_amd.probe_labeler import ProbeLabeler
    folder = EC.build_labeler_probes(str(tmp_path / "probe_positive"))
    meta = str(tmp_path / "probe_positive_metadata.json")
    with open(meta, "w") as f:
        json.dump(EC.LABELER_METADATA, f, indent=2)
    gallery = GalleryManager(gallery_path=str(tmp_path / "gallery" / "students.pkl"), device=emb.device, verbose=False)
    for (sid, name), row in zip(EC.STUDENTS, golden["labeler__real__gallery_rows"]):
        gallery.add_student(sid, name, row)
    lab = ProbeLabeler(None, EC.MODEL_TYPE, EC.ARCHITECTURE, embedder=emb, gallery=gallery, verbose=False,
                       block_images=3)
    dst = str(tmp_path / "labeled")
    summary = lab.process_probe_directory(folder, output_dir=dst, metadata_file=meta, top_k=EC.TOP_K)
    with open(os.path.join(dst, "labeling_results.json")) as f:
        doc = EC.strip_labeling(json.load(f), dst)
    want = json.loads(str(golden["labeler__real__doc"]))
    assert {k: v for k, v in summary.items() if k != "timestamp"} == want["summary"]
    assert EC.copied_names(dst) == json.loads(str(golden["labeler__real__copied"]))
    assert [r["filename"] for r in doc["results"]] == [r["filename"] for r in want["results"]]
    worst = 0.0
    for got, ref in zip(doc["results"], want["results"]):
        assert list(got) == list(ref)
        for key in ("matched_student_id", "matched_name", "label", "original_metadata", "labeled_path"):
            assert got[key] == ref[key], (got["filename"], key)
        assert [(m["student_id"], m["name"], m["rank"]) for m in got["top_matches"]] == \
               [(m["student_id"], m["name"], m["rank"]) for m in ref["top_matches"]], got["filename"]
        worst = max([worst, abs(got["confidence"] - ref["confidence"])] +
                    [abs(a["score"] - b["score"]) for a, b in zip(got["top_matches"], ref["top_matches"])])
    print("ProbeLabeler vs the reference: max abs score difference", worst)
    assert worst <= SCORE_TOL
