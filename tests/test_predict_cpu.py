"""The host side of prediction, without a GPU: KGC.describe_entities / describe_relations on the MARS fixtures (tests/golden/mars) and
Trainer.predict's concatenation, row offsets and eval-mode call with a stub lit model."""
import argparse
import json
import os
import shutil

import numpy as np
import pytest
import torch

from mkg_analogy_amd.data import BertWordPieceTokenizer
from mkg_analogy_amd.data.data_module import KGC

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "mars")
G6 = np.load(os.path.join(HERE, "golden", "g6_mars_plumbing.npz"))


@pytest.fixture(scope="module")
def dm(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("mars_predict")
    data_dir, pre = tmp / "MARS", tmp / "MarKG"
    data_dir.mkdir(); pre.mkdir()
    for fn in ("dev.json", "train.json", "test.json", "analogy_entities.txt", "analogy_relations.txt"):
        shutil.copy(os.path.join(FIX, fn), data_dir)
    for fn in ("entity2text.txt", "relation2text.txt", "wiki_tuple_ids.txt"):
        shutil.copy(os.path.join(FIX, fn), pre)
    args = argparse.Namespace(model_name_or_path="bert-base-uncased", data_dir=str(data_dir), pretrain_path=str(pre), pretrain=0, max_seq_length=64,
                              overwrite_cache=True, precision=32, model_class="MKGformerKGC", batch_size=8, eval_batch_size=8, num_workers=0)
    n = sum(1 for _ in open(os.path.join(FIX, "entity2text.txt")))
    m = KGC(args, None, tokenizer=BertWordPieceTokenizer(G6["vocab"].tolist()), visual_features=torch.zeros(n, 3, 2, 2))
    m.setup()
    return m


def _pairs(fn):
    with open(os.path.join(FIX, fn), encoding="utf-8") as f:
        return [line.rstrip("\n").split("\t", 1) for line in f]


def _dev_lines():
    with open(os.path.join(FIX, "dev.json"), encoding="utf-8") as f:
        txt = f.read()
    try:
        data = json.loads(txt)
        return data if isinstance(data, list) else [data]
    except json.JSONDecodeError:
        return [json.loads(line) for line in txt.splitlines() if line.strip()]


# get_config() after setup(): every instance attribute whose name contains "st", "ed" or "analogy" (the reference's filter picks up two bystanders)
CONFIG_KEYS = {"label_list", "data_test", "relation_id_st", "relation_id_ed", "entity_id_st", "entity_id_ed", "analogy_entity_ids", "analogy_relation_ids"}


def test_describe_entities_gives_back_every_dev_answer(dm):
    keys_before = set(dm.get_config())
    lines = _dev_lines()
    labels = [f["label"] for f in dm.data_val.features]
    assert len(lines) == len(labels) == 1020
    text = dict(_pairs("entity2text.txt"))
    for line, label in zip(lines, labels):
        (d,) = dm.describe_entities([label])
        assert d == {"index": label, "key": line["answer"], "text": text[line["answer"]]}
    got = dm.describe_entities(torch.tensor(labels[:50]))                       # a tensor (a row of entity_topk) works as a list does
    assert [d["key"] for d in got] == [line["answer"] for line in lines[:50]]
    assert [d["key"] for d in dm.describe_entities(np.array([[labels[0], labels[1]]]))] == [lines[0]["answer"], lines[1]["answer"]]
    assert set(dm.get_config()) == keys_before == CONFIG_KEYS                    # nothing was cached under a name get_config() picks up


def test_describe_entities_inverts_the_tables(dm):
    t = dm.processor.tables(dm.args.data_dir)
    ents = _pairs("entity2text.txt")
    assert len(t.ent2id) == len(ents) == 11292
    probe = list(range(0, len(ents), 97)) + [len(ents) - 1]
    for i, d in zip(probe, dm.describe_entities(probe, space="entity")):
        assert d["key"] == ents[i][0] and d["text"] == ents[i][1] and t.ent2id[d["key"]] == i == d["index"]
    n = len(t.analogy_ent2id)
    assert n == len(dm.analogy_entity_ids) == 2063
    for i, d in enumerate(dm.describe_entities(range(n))):
        assert t.analogy_ent2id[d["key"]] == i
        assert dm.tokenizer.get_added_vocab()[f"[ENTITY_{t.ent2id[d['key']]}]"] == dm.analogy_entity_ids[i]      # the token the head scores at column i
    for bad in ([-1], [n], [11292]):
        with pytest.raises(IndexError):
            dm.describe_entities(bad, space="analogy" if bad != [11292] else "entity")
    with pytest.raises(ValueError):
        dm.describe_entities([0], space="relation")


def test_describe_relations(dm):
    t = dm.processor.tables(dm.args.data_dir)
    rels = _pairs("relation2text.txt")
    got = dm.describe_relations(range(len(rels)), space="relation")
    assert [(d["key"], d["text"]) for d in got] == [(k, v) for k, v in rels]
    vocab = dm.tokenizer.get_added_vocab()
    keys = [k for k, _ in rels]
    for i, d in enumerate(dm.describe_relations(range(len(dm.analogy_relation_ids)))):
        assert t.rel2id[d["key"]] == i                                            # the analogy numbering of rel2id
        assert vocab[f"[RELATION_{keys.index(d['key'])}]"] == dm.analogy_relation_ids[i]
    with pytest.raises(IndexError):
        dm.describe_relations([len(rels)], space="relation")
    assert set(dm.get_config()) == CONFIG_KEYS


class _StubModel:
    def __init__(self):
        self.training = True

    def eval(self):
        self.training = False


class _StubLit:
    """predict_step of a pre-train lit model: even examples ask for an entity, odd ones for a relation."""

    def __init__(self):
        self.model, self.calls = _StubModel(), []

    def predict_step(self, batch, batch_idx, k=None):
        assert not self.model.training
        ids = batch["input_ids"]
        self.calls.append((batch_idx, k, int(ids.shape[0])))
        tag = ids[:, 0].numpy()
        local = np.arange(len(tag))
        ent, rel = local[tag % 2 == 0], local[tag % 2 == 1]
        out = {}
        if len(ent):
            out.update(entity_rows=ent, entity_topk=np.repeat(tag[ent][:, None], k, 1).astype(np.int64), entity_topk_logits=np.full((len(ent), k), 0.5, np.float32))
        if len(rel):
            out.update(relation_rows=rel, relation_topk=np.repeat(tag[rel][:, None], k, 1).astype(np.int64), relation_ranks=tag[rel].astype(np.int64))
        batch.pop("input_ids")                                                       # a hook may consume its batch: the loader's dict must survive
        return out


def test_trainer_predict_concatenates_and_offsets_rows(monkeypatch):
    from mkg_analogy_amd import functional as Fn
    from mkg_analogy_amd.trainer import Trainer
    checks = []
    monkeypatch.setattr(Fn, "check_status", lambda: checks.append(1))
    sizes = [3, 1, 4]
    tags = np.arange(sum(sizes))
    batches, s = [], 0
    for n in sizes:
        batches.append({"input_ids": torch.from_numpy(tags[s:s + n])[:, None].repeat(1, 5)})
        s += n
    lit = _StubLit()
    out = Trainer(world_size=1).predict(lit, batches, k=2)
    assert lit.calls == [(0, 2, 3), (1, 2, 1), (2, 2, 4)] and lit.model.training is False
    assert checks == [1]                                                             # one status check for the whole pass
    assert all("input_ids" in b for b in batches)
    assert out["entity_rows"].tolist() == [0, 2, 4, 6] and out["relation_rows"].tolist() == [1, 3, 5, 7]      # batch-global
    assert out["entity_topk"].tolist() == [[t, t] for t in (0, 2, 4, 6)] and out["relation_topk"][:, 0].tolist() == [1, 3, 5, 7]
    assert out["relation_ranks"].tolist() == [1, 3, 5, 7] and out["entity_topk_logits"].shape == (4, 2)
    assert "entity_ranks" not in out
    assert Trainer(world_size=1).predict(_StubLit(), [], k=2) == {}
