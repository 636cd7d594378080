import torch
import torch.nn as nn

from ... import _native
from .Model import Model


class TransD(Model):
    """TransD (openke/module/model/TransD.py:6-155) with dim_e == dim_r: every entity and relation carries a
    transfer vector, an entity is scored as normalize(e + (e . e_transfer) r_transfer) and then as in TransE. Same
    constructor signature, attribute names and initialisation order as the reference (four nn.Embedding tables, then
    their four xavier / uniform inits); scoring and training run in the HIP kernels (transd.hip). dim_e != dim_r is
    refused: the reference's own _resize fails there for dim_e < dim_r (its F.pad call passes a keyword torch does not
    have)."""

    native_model = _native.PT_TRANSD

    def __init__(self, ent_tot, rel_tot, dim_e=100, dim_r=100, p_norm=1, norm_flag=True, margin=None, epsilon=None):
        super(TransD, self).__init__(ent_tot, rel_tot)
        if dim_e != dim_r:
            raise NotImplementedError("TransD with dim_e != dim_r (%d, %d) is outside the accelerated path"
                                      % (dim_e, dim_r))
        self.dim_e = dim_e
        self.dim_r = dim_r
        self.margin = margin
        self.epsilon = epsilon
        self.norm_flag = norm_flag
        self.p_norm = p_norm
        self.ent_embeddings = self._embedding(self.ent_tot, self.dim_e)
        self.rel_embeddings = self._embedding(self.rel_tot, self.dim_r)
        self.ent_transfer = self._embedding(self.ent_tot, self.dim_e)
        self.rel_transfer = self._embedding(self.rel_tot, self.dim_r)
        if margin is None or epsilon is None:
            self._xavier_uniform_(self.ent_embeddings.weight.data)
            self._xavier_uniform_(self.rel_embeddings.weight.data)
            self._xavier_uniform_(self.ent_transfer.weight.data)
            self._xavier_uniform_(self.rel_transfer.weight.data)
        else:
            self.ent_embedding_range = nn.Parameter(torch.Tensor([(self.margin + self.epsilon) / self.dim_e]),
                                                    requires_grad=False)
            self.rel_embedding_range = nn.Parameter(torch.Tensor([(self.margin + self.epsilon) / self.dim_r]),
                                                    requires_grad=False)
            er, rr = self.ent_embedding_range.item(), self.rel_embedding_range.item()
            self._uniform_(self.ent_embeddings.weight.data, -er, er)
            self._uniform_(self.rel_embeddings.weight.data, -rr, rr)
            self._uniform_(self.ent_transfer.weight.data, -er, er)
            self._uniform_(self.rel_transfer.weight.data, -rr, rr)
        if margin is not None:
            self.margin = nn.Parameter(torch.Tensor([margin]))
            self.margin.requires_grad = False
            self.margin_flag = True
        else:
            self.margin_flag = False

    def tables(self):
        """(ent, rel, None, ent_transfer, rel_transfer) weight tensors."""
        return (self.ent_embeddings.weight, self.rel_embeddings.weight, None, self.ent_transfer.weight,
                self.rel_transfer.weight)

    def forward(self, data):
        score = self.native_score(data)
        if self.margin_flag:
            return self.margin - score
        return score

    def regularization(self, data):
        raise NotImplementedError("regularisation is outside the accelerated path (regul_rate is 0 in every config)")

    def predict(self, data):
        score = self.forward(data)
        if self.margin_flag:
            score = self.margin - score
        return score.cpu().data.numpy()
