"""Drop-in `models.lightgcn_fusion.LightGCN_Fusion` (reference models/lightgcn_fusion.py:5-64).

Same constructor (raises without pretrained content embeddings), module registration and RNG
order (user, item_id, brand embeddings, fusion Linear, then four xavier inits), buffer
`item_content_embedding`, and 5-tuple. The item pre-fusion `leaky_relu(Linear([id ‖ content]))`
(lightgcn_fusion.py:45-49) runs as one engine kernel on a HIP device (no concatenation, MFMA GEMM
with bias + leaky_relu fused, gcn_recommendation_amd.fusion); the K-layer
propagation + mean (lightgcn_fusion.py:55-59) runs in the MI355X engine, reading
E0 = [user | fused_item | brand] as three segments.
"""
import torch
import torch.nn as nn

from gcn_recommendation_amd import engine, fusion, train


class LightGCN_Fusion(nn.Module):
    def __init__(self, num_users, num_items, num_brands, config, pretrained_item_emb=None):
        super(LightGCN_Fusion, self).__init__()
        self.num_users = num_users
        self.num_items = num_items
        self.num_brands = num_brands
        self.embedding_dim = config.embedding_dim
        self.n_layers = config.n_layers
        if pretrained_item_emb is None:
            raise ValueError("LightGCN_Fusion model requires pretrained item embeddings.")
        content_emb_dim = pretrained_item_emb.shape[1]
        self.user_embedding = nn.Embedding(num_users, self.embedding_dim)
        self.item_id_embedding = nn.Embedding(num_items, self.embedding_dim)
        self.brand_embedding = nn.Embedding(num_brands, self.embedding_dim)
        self.register_buffer('item_content_embedding', torch.FloatTensor(pretrained_item_emb))
        self.item_fusion_layer = nn.Linear(self.embedding_dim + content_emb_dim, self.embedding_dim)
        nn.init.xavier_uniform_(self.user_embedding.weight)
        nn.init.xavier_uniform_(self.item_id_embedding.weight)
        nn.init.xavier_uniform_(self.brand_embedding.weight)
        nn.init.xavier_uniform_(self.item_fusion_layer.weight)
        self._graph_adj = None

    def fused_item_embedding(self):
        # lightgcn_fusion.py:45-49; on a HIP device one engine kernel (gcn_recommendation_amd.fusion)
        return fusion.fused_item_embedding(self.item_id_embedding.weight,
                                           self.item_content_embedding, self.item_fusion_layer)

    def forward(self, adj_mat, use_brand=True):
        user_emb_0 = self.user_embedding.weight
        item_id_emb_0 = self.item_id_embedding.weight
        brand_emb_0 = self.brand_embedding.weight
        fused_item_emb_0 = self.fused_item_embedding()
        segments = [user_emb_0, fused_item_emb_0, brand_emb_0]
        if adj_mat.device.type == "cuda":
            # user_emb_0 as the engine's alias: its gradient joins the propagation's inside the
            # backward (engine.PropagateFunction, e0_outputs)
            final_user_emb, final_item_emb, final_brand_emb, user_emb_0 = engine.propagate_blocks(
                adj_mat, segments, self.n_layers, e0_outputs=1)
        else:  # CPU adjacency: the reference's ATen path (lightgcn_fusion.py:52-59)
            ego = torch.cat(segments, dim=0)
            all_embeddings = [ego]
            for _ in range(self.n_layers):
                ego = torch.sparse.mm(adj_mat, ego)
                all_embeddings.append(ego)
            final_embeddings = torch.mean(torch.stack(all_embeddings, dim=0), dim=0)
            final_user_emb, final_item_emb, final_brand_emb = torch.split(
                final_embeddings, [self.num_users, self.num_items, self.num_brands])
        return final_user_emb, final_item_emb, final_brand_emb, user_emb_0, item_id_emb_0

    _bpr_n_e0 = 1  # only the user rows: the item segment is the pre-layer's output

    def bpr_step(self, adj, users, pos, neg, lambda_reg, *, item_brand=None,
                 brand_loss_weight=0.1, negatives="hardest", return_negatives=False,
                 temperature=1.0, neg_log_q=None):
        """The BPR + L2 loss of one batch in one call that keeps the batch indices
        (train.bpr_step): the item segment is the pre-layer's output and keeps its autograd
        graph, the item regulariser rows come from item_id_embedding.weight. A [B, M] neg holds
        M candidate negatives per sample (negatives="hardest", "all" or "softmax" with its
        `temperature` and `neg_log_q`, as LightGCN.bpr_step)."""
        return train.bpr_step(self, adj, users, pos, neg, lambda_reg, item_brand=item_brand,
                              brand_loss_weight=brand_loss_weight, negatives=negatives,
                              return_negatives=return_negatives, temperature=temperature,
                              neg_log_q=neg_log_q)

    def inbatch_step(self, adj, users, pos, lambda_reg, temperature=1.0, *, positives=None,
                     item_log_q=None, check_indices=False):
        """The in-batch softmax + L2 loss of one batch (train.inbatch_step), as
        LightGCN.inbatch_step: the item segment is the pre-layer's output, the item regulariser
        rows come from item_id_embedding.weight."""
        return train.inbatch_step(self, adj, users, pos, lambda_reg, temperature,
                                  positives=positives, item_log_q=item_log_q,
                                  check_indices=check_indices)

    def bpr_epoch(self, adj, sampler, optimizer, lambda_reg, batch_size, epoch, shuffle=True,
                  item_brand=None, brand_loss_weight=0.1, n_neg=None, negatives="hardest",
                  temperature=1.0, *, mask_positives=False, log_q=False, neg_log_q=False):
        """One epoch of bpr_step batches over one device-side draw of the sampler
        (train.bpr_epoch): the per-batch losses as one tensor, no host read-back in the loop.
        `gcn_recommendation_amd.optim.Adam` as the optimizer keeps the whole step inside the
        engine, with torch.optim.Adam's bits. n_neg = M draws M candidate negatives per sample
        for bpr_step's `negatives` mode; negatives="in_batch" (n_neg=None) runs inbatch_step on
        every batch, with mask_positives / log_q taken from the sampler; neg_log_q=True gives
        the "softmax" steps the sampler's neg_log_q()."""
        return train.bpr_epoch(self, adj, sampler, optimizer, lambda_reg, batch_size, epoch,
                               shuffle=shuffle, item_brand=item_brand,
                               brand_loss_weight=brand_loss_weight, n_neg=n_neg,
                               negatives=negatives, temperature=temperature,
                               mask_positives=mask_positives, log_q=log_q,
                               neg_log_q=neg_log_q)

    def evaluate_ranks(self, adj, evaluator, eval_users, eval_items, ks=(20,)):
        """Recall@k / NDCG@k for every k of `ks` and MRR from one device-side pass
        (evaluate.Evaluator: the held-out item's exact rank per user, one read-back)."""
        return evaluator.evaluate(self, adj, (eval_users, eval_items), ks)

    def evaluate_rank_lists(self, adj, evaluator, eval_users, eval_items, ks=(20,)):
        """Recall / precision / hit / NDCG @k and MRR over every held-out item of every user
        (evaluate.Evaluator.evaluate_lists: all (user, item) rows are kept, one read-back)."""
        return evaluator.evaluate_lists(self, adj, (eval_users, eval_items), ks)

    def recommend(self, adj, users, k, evaluator, batch_size=8192, exclude_train=True):
        """The k best items per user in rank order, (scores fp32, items int32) [n x k] on the
        device, for k up to evaluate.WIDE_MAX_K on the kernel (evaluate.Evaluator.recommend)."""
        return evaluator.recommend(self, adj, users, k, batch_size, exclude_train)

    def set_graph(self, adj_mat):
        self._graph_adj = adj_mat
        return self

    def computer(self, adj_mat=None):
        adj = adj_mat if adj_mat is not None else self._graph_adj
        if adj is None:
            raise ValueError("computer() needs adj_mat (or set_graph(adj_mat) first)")
        fu, fi, _, _, _ = self.forward(adj)
        return fu, fi
