#!/usr/bin/env python
"""TEST INFRASTRUCTURE (needs the reference checkout; see oracle/ref_import.py).  Captures tests/golden/char_embeddings.npz by RUNNING
THE REFERENCE's FastCharacterEmbeddings and ColumnDataLoader._get_char_idx:   python tools/gen_golden_char.py

A handful of sentences (characters outside the dictionary, a one-character word, repeated words, sentences of different lengths) and
seeded weights.  Recorded: the vocabulary handed to the constructor, the dictionary (its items in order, their ids), the sentences,
char_seqs [Lmax, B * n] and char_lengths [B * n] as ColumnDataLoader.assign_embeddings lays them out (flair/custom_data_loader.py
:150-197: padding positions hold id 0 with length 1), the state dict, the features [B, n, 50] of embed_sentences, a fixed weight tensor
G [B, n, 50] that is zero at the padding positions, and the gradients of sum(features * G) with respect to every parameter.
Data only: inputs and the reference's outputs."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
GOLD = os.path.join(ROOT, "tests", "golden")

from oracle import ref_import  # noqa: E402

VOCAB = ["alice", "visited", "berlin", "the", "museum", "of", "art", "a", "bob", "wikipedia", "alice"]
TEXTS = ["alice visited berlin", "a", "bob saw the quiz of alice alice", "Art a museum"]      # 's', 'w' in the dictionary; q, z, A are not


def main():
    ref_import.load_reference()
    import flair
    from flair.custom_data_loader import ColumnDataLoader
    from flair.data import Sentence as RS
    from flair.embeddings import FastCharacterEmbeddings as Ref
    flair.device = torch.device("cpu")
    torch.manual_seed(1234)
    emb = Ref(vocab=VOCAB)
    sents = [RS(t) for t in TEXTS]
    B, n = len(sents), max(len(s) for s in sents)
    Lmax = max(len(w.text) for s in sents for w in s)
    char_tensor = torch.zeros([B, n, Lmax]).long()
    char_length = torch.ones([B, n]).long()
    for b, s in enumerate(sents):
        chars, lens = ColumnDataLoader._get_char_idx(None, emb.char_dictionary, s)
        char_tensor[b][:len(s), :chars.shape[0]] = chars.transpose(0, 1)
        char_length[b][:len(s)] = lens

    class Batch(list):
        pass
    bt = Batch(sents)
    bt.char_seqs, bt.char_lengths, bt.max_sent_len = char_tensor.reshape(-1, Lmax).transpose(1, 0), char_length.reshape(-1), n
    feats = emb.embed_sentences(bt)
    rng = np.random.default_rng(7)
    G = rng.standard_normal((B, n, feats.shape[-1]))
    for b, s in enumerate(sents):
        G[b, len(s):] = 0.0
    (feats.double() * torch.from_numpy(G)).sum().backward()
    out = {"vocab": np.asarray(VOCAB), "texts": np.asarray(TEXTS), "dict_items": np.asarray(list(emb.char_dictionary.keys())),
           "dict_ids": np.asarray(list(emb.char_dictionary.values()), np.int64), "char_seqs": bt.char_seqs.numpy(),
           "char_lengths": bt.char_lengths.numpy(), "features": feats.detach().numpy().astype(np.float32), "G": G,
           "embedding_length": np.int64(emb.embedding_length), "name": np.asarray(emb.name)}
    for k, v in emb.state_dict().items():
        out["state/" + k] = v.detach().numpy()
    for k, p in emb.named_parameters():
        out["grad/" + k] = p.grad.numpy().astype(np.float64)
    path = os.path.join(GOLD, "char_embeddings.npz")
    np.savez_compressed(path, **out)
    print("  char_embeddings.npz %d bytes, %d arrays" % (os.path.getsize(path), len(out)))


if __name__ == "__main__":
    main()
