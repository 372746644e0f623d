#!/usr/bin/env python3
"""Device time of one KeyFrameDatabase query (DetectRelocalizationCandidates and DetectLoopCandidates, the _device
forms: share pass, threshold, score pass, candidate pass) at two sizes:
  2,000 keyframes x ~1,000 words (a long session's database; the candidate pass sorts in LDS),
  kKfdbLdsSort + 1 = 2,049 keyframes of the same shape (the first slot count whose candidate pass sorts in global scratch).
BowVectors are drawn around shared prototypes over a flat 100,000-word vocabulary (~70 % of a prototype's 1,300
words plus 100 random ones), the query the same way; covisibility rows are random.  HIP events around 200 queries
after 20 warm-ups, three repeats; device time only: there is no compiled reference for this path to compare with.
Prints one JSON line per size and form.
  python tools/diag/kfdb_query.py            (on the GPU box)"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [os.path.join(ROOT, "orb-slam-_amd")]
import orbx  # noqa: E402

NWORDS = 100000
KFDB_LDS_SORT = 2048   # orbx_kfdb.hip kKfdbLdsSort


def bow(rng, protos):
    p = protos[int(rng.integers(len(protos)))]
    w = np.unique(np.concatenate([p[rng.random(len(p)) < 0.7], rng.integers(0, NWORDS, 100)])).astype(np.int32)
    v = 10.0 ** rng.uniform(-3, 3, len(w))
    return w, v / v.sum()


def main():
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    parent = np.zeros(NWORDS + 1, np.int32)
    leaf = np.ones(NWORDS + 1, np.uint8)
    leaf[0] = 0
    voc = orbx.ORBVocabulary.from_arrays(NWORDS, 1, parent, leaf, np.zeros((NWORDS + 1, 32), np.uint8),
                                         np.ones(NWORDS + 1))
    protos = [rng.choice(NWORDS, 1300, replace=False) for _ in range(8)]
    for nkf in (2000, KFDB_LDS_SORT + 1):
        kfs = [bow(rng, protos) for _ in range(nkf)]
        cap = max(len(w) for w, _ in kfs)
        bw = np.zeros((nkf, cap), np.int32)
        bv = np.zeros((nkf, cap), np.float64)
        for i, (w, v) in enumerate(kfs):
            bw[i, :len(w)], bv[i, :len(w)] = w, v
        bn = np.array([len(w) for w, _ in kfs], np.int32)
        db = orbx.KeyFrameDatabase(voc, reserve_keyframes=nkf, reserve_words=int(bn.sum()))
        db.add_batch_device(torch.from_numpy(bw).to(dev), torch.from_numpy(bv).to(dev), torch.from_numpy(bn).to(dev))
        covis = torch.from_numpy(rng.integers(-1, nkf, (nkf, 10)).astype(np.int32)).to(dev)
        conn = torch.from_numpy((rng.random(nkf) < 0.01).astype(np.uint8)).to(dev)
        qw, qv = bow(rng, protos)
        q_word, q_weight = torch.from_numpy(qw).to(dev), torch.from_numpy(qv).to(dev)
        q_n = torch.tensor([len(qw)], dtype=torch.int32, device=dev)
        # the C entry points on preallocated outputs: one ctypes call per query, so the events time the stream's work
        cand = torch.empty(nkf, dtype=torch.int32, device=dev)
        nc = torch.empty(1, dtype=torch.int32, device=dev)
        words = torch.empty(nkf, dtype=torch.int32, device=dev)
        sc = torch.empty(nkf, dtype=torch.float32, device=dev)
        P = lambda t: C.c_void_p(t.data_ptr())
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        L = orbx.lib
        forms = {"reloc": lambda: L.orbv_db_detect_reloc_device(db._h, P(q_word), P(q_weight), P(q_n), len(qw),
                                                                P(covis), nkf, P(cand), P(nc), P(words), P(sc), st),
                 "loop": lambda: L.orbv_db_detect_loop_device(db._h, P(q_word), P(q_weight), P(q_n), len(qw), P(conn),
                                                              P(covis), 0.02, nkf, P(cand), P(nc), P(words), P(sc),
                                                              st)}
        for name, run in forms.items():
            for _ in range(20):
                assert run() == orbx.OK
            torch.cuda.synchronize()
            ms = []
            for _ in range(3):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(200):
                    run()
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1) / 200)
            minc = int(np.float32(int(words.max())) * np.float32(0.8))
            print(json.dumps({"keyframes": nkf, "words_per_keyframe": round(float(bn.mean()), 1), "query_words": len(qw),
                              "form": name, "ms_per_query": [round(m, 4) for m in ms],
                              "index_MB": round(int(bn.sum()) * 12 / 1e6, 1),
                              "scored": int((words > minc).sum()), "candidates": int(nc),
                              "sort": "LDS" if nkf <= KFDB_LDS_SORT else "global"}), flush=True)
        db.close()


if __name__ == "__main__":
    main()
