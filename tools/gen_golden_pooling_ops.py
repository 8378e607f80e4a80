#!/usr/bin/env python
"""TEST INFRASTRUCTURE (needs the reference checkout; see oracle/ref_import.py).  Captures tests/golden/pooling_ops.npz by RUNNING THE
REFERENCE's TransformerWordEmbeddings, frozen, under every pooling operation:   python tools/gen_golden_pooling_ops.py

The two tiny models and the crafted texts of G7 (oracle/gen_golden_e2e.py: a sentencepiece-style and a BERT-style tokenizer, word tokens
the tokenizer drops, a long word clamped by maximum_subtoken_length, <EOS>).  Per tokenizer (`sp/`, `wp/`): texts, n_tokens,
maximum_subtoken_length, ids, mask, hidden [L + 1, B, S, H] (every hidden state, captured once -- the weights do not depend on the
pooling) and, for each of first / last / first_last / mean x use_scalar_mix off / on at layers='-1,-2', the reference's
features [B, n, W] under `feat/<op>/<cat|mix>`.  Data only: inputs and the reference's outputs."""
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
GOLD = os.path.join(ROOT, "tests", "golden")

from oracle import ref_import  # noqa: E402
from oracle.gen_golden_e2e import patch_model_dir  # noqa: E402

LAYERS = "-1,-2"
OPS = ("first", "last", "first_last", "mean")
TEXTS = {"sp": (["alice visited \u00ad berlin <EOS> the museum of art", "zalandoresearchuniversitycambridge is located in berlin",
                 "bob <EOS> wikipedia"], 3),
         "wp": (["alice visited \x01 berlin <EOS> the museum of art", "\x01 zalandoresearchuniversity works \x02",
                 "bob <EOS> wikipedia"], 4)}


def main():
    ref_import.load_reference()
    ref_import.wrap_auto_tokenizer()
    import tiny_assets
    import transformers
    _orig_am = transformers.AutoModel.from_pretrained
    transformers.AutoModel.from_pretrained = staticmethod(lambda *a, **k: _orig_am(*a, attn_implementation="eager", **k))
    from flair.custom_data_loader import BatchedData
    from flair.data import Sentence as RS
    from flair.embeddings import TransformerWordEmbeddings as RefTWE

    work = tempfile.mkdtemp(prefix="poolops_")
    dirs = {"sp": tiny_assets.build_model_dir(os.path.join(work, "xlmr-tiny")),
            "wp": tiny_assets.build_model_dir(os.path.join(work, "bert-tiny"), tokenizer="wordpiece", seed=3)}
    out, failed = {}, []
    for kind, mdir in dirs.items():
        patch_model_dir(mdir)
        texts, max_sub = TEXTS[kind]
        out[kind + "/texts"] = np.asarray(texts)
        out[kind + "/maximum_subtoken_length"] = np.int64(max_sub)
        for op in OPS:
            for mix in (False, True):
                tag = "%s/feat/%s/%s" % (kind, op, "mix" if mix else "cat")
                try:
                    emb = RefTWE(model=mdir, layers=LAYERS, pooling_operation=op, use_scalar_mix=mix, fine_tune=False)
                    emb.eval()
                    emb.maximum_subtoken_length = max_sub
                    sents = [RS(t) for t in texts]
                    batch = BatchedData(sents)
                    cap = {}
                    fwd = emb.model.forward

                    def spy(input_ids, attention_mask=None, _fwd=fwd, _cap=cap, **k):
                        o = _fwd(input_ids, attention_mask=attention_mask, **k)
                        _cap["ids"], _cap["mask"] = input_ids.clone(), attention_mask.clone()
                        _cap["hidden"] = torch.stack([h.detach() for h in o[2]])
                        return o

                    emb.model.forward = spy
                    with torch.no_grad():
                        emb.embed(batch)
                    emb.model.forward = fwd
                    feats = batch.features[emb.name].detach().numpy()
                except Exception as e:    # a combination the reference cannot run under the shims: reported, the others are kept
                    failed.append((tag, repr(e)))
                    continue
                out[tag] = feats.astype(np.float32)
                got = {"ids": cap["ids"].numpy(), "mask": cap["mask"].numpy(), "hidden": cap["hidden"].numpy().astype(np.float32),
                       "n_tokens": np.asarray([len(s) for s in sents])}
                for k, v in got.items():
                    if kind + "/" + k in out:
                        assert np.array_equal(out[kind + "/" + k], v), (tag, k)     # the encoder half does not depend on the pooling
                    out[kind + "/" + k] = v
    path = os.path.join(GOLD, "pooling_ops.npz")
    np.savez_compressed(path, **out)
    shutil.rmtree(work, ignore_errors=True)
    print("  pooling_ops.npz %d bytes, %d arrays" % (os.path.getsize(path), len(out)))
    for tag, err in failed:
        print("  NOT CAPTURED %s: %s" % (tag, err))


if __name__ == "__main__":
    main()
