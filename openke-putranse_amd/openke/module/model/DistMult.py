import torch
import torch.nn as nn

from ... import _native
from .Model import Model


class DistMult(Model):
    """DistMult (openke/module/model/DistMult.py:5-72): a triple is scored by sum_j h_j r_j t_j, higher is better;
    forward returns the score, predict its negative. Same constructor signature, attribute names, state_dict keys and
    initialisation order as the reference (two nn.Embedding tables, then xavier on both, or uniform(+-(margin +
    epsilon) / dim) on both when margin and epsilon are given - they only choose the init, no margin enters the score),
    so a seeded construction gives the reference's tables. Scores and training run in the HIP kernels (distmult.hip);
    there is no tensor-level _calc. The two regularisers are computed inside the native step
    (NegativeSampling(regul_rate=, l3_regul_rate=)); regularization() and l3_regularization() return the reference's
    values from the tables."""

    native_model = _native.PT_DISTMULT
    p_norm, norm_flag = 1, False   # (fields of the native descriptor the DistMult kernels do not read)

    def __init__(self, ent_tot, rel_tot, dim=100, margin=None, epsilon=None):
        super(DistMult, self).__init__(ent_tot, rel_tot)
        self.dim = dim
        self.margin = margin
        self.epsilon = epsilon
        self.ent_embeddings = self._embedding(self.ent_tot, self.dim)
        self.rel_embeddings = self._embedding(self.rel_tot, self.dim)
        if margin is None or epsilon is None:
            self._xavier_uniform_(self.ent_embeddings.weight.data)
            self._xavier_uniform_(self.rel_embeddings.weight.data)
        else:
            self.embedding_range = nn.Parameter(torch.Tensor([(self.margin + self.epsilon) / self.dim]),
                                                requires_grad=False)
            self._uniform_(self.ent_embeddings.weight.data, -self.embedding_range.item(),
                           self.embedding_range.item())
            self._uniform_(self.rel_embeddings.weight.data, -self.embedding_range.item(),
                           self.embedding_range.item())

    def forward(self, data):
        return -self.native_score(data)

    def _rows(self, data):
        dev = self.ent_embeddings.weight.device
        return (self.ent_embeddings(self._ids(data['batch_h'], dev)), self.ent_embeddings(self._ids(data['batch_t'], dev)),
                self.rel_embeddings(self._ids(data['batch_r'], dev)))

    def regularization(self, data):
        h, t, r = self._rows(data)
        return (torch.mean(h ** 2) + torch.mean(t ** 2) + torch.mean(r ** 2)) / 3

    def l3_regularization(self):
        return self.ent_embeddings.weight.norm(p=3) ** 3 + self.rel_embeddings.weight.norm(p=3) ** 3

    def predict(self, data):
        score = -self.forward(data)
        return score.cpu().data.numpy()
