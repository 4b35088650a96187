"""Worker of tests/test_grad_clip_gpu.py::test_one_rank_process_group_with_clipping_matches_the_plain_run (launched with torch.distributed.run, one
rank, MART_FORCE_PG=1).  Two clipped train_steps of the same seeded MKGformer from the same weights: one with the bucketed, backward-overlapped
all-reduce of the 1-rank nccl group in front of the clip, one with the reducer off.  A sum over one rank is the identity and the norm is taken after
``sync.finish()``, so norm, coefficient and masters must agree bit for bit.  Prints one JSON line."""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    import bench
    from mkg_analogy_amd import data_synth as D
    from mkg_analogy_amd.distributed import init_from_env
    from mkg_analogy_amd.trainer import Trainer
    rank, local, world = init_from_env()
    assert world == 1 and torch.distributed.is_initialized()
    model, lit, cfg = bench.build(32, seed=0, device=torch.device("cuda", local), backbone="mkgformer")
    D.load_seeded_weights(model, lit, seed=3, conditioned=True)
    lit.args.warm_up_radio = 0.0                                        # a non-zero learning rate from the first step on
    model.finalize()
    st = model.store
    w0 = st.master.detach().clone()
    batch = D.make_batch(4, 57, seed=100, device="cuda")

    def run(force_pg, clip):
        os.environ["MART_FORCE_PG"] = "1" if force_pg else "0"
        with torch.no_grad():
            st.master.copy_(w0)
        st.refresh_shadows()
        st.zero_grad()
        model._step = 0
        model.engine.grad_ready = model.engine.grad_ready_async = None
        tr = Trainer(max_epochs=1, world_size=1, gradient_clip_val=clip, track_grad_norm=None if clip else 2)
        tr._setup(lit, [batch] * 4)
        tr.train_step(lit, batch, 0)
        torch.cuda.synchronize()
        coef = tr.optimizer.last_clip_coef
        return tr.sync.reducer is not None, float(tr.optimizer.last_grad_norm), None if coef is None else float(coef), st.master.detach().clone()

    _, norm0, _, _ = run(False, None)
    on, norm_pg, coef_pg, m_pg = run(True, 0.5 * norm0)
    off, norm_plain, coef_plain, m_plain = run(False, 0.5 * norm0)
    print(json.dumps({"reducer_on": on, "reducer_off": off, "norm_pg": norm_pg, "norm_plain": norm_plain, "coef_pg": coef_pg, "coef_plain": coef_plain,
                      "masters_equal": bool(torch.equal(m_pg, m_plain)), "moved": int((m_pg != w0).sum())}))
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
