import torch
import torch.nn as nn

from ... import _native
from .Model import Model


class RotatE(Model):
    """RotatE (openke/module/model/RotatE.py:6-103): an entity is dim complex numbers (a row of 2 * dim floats,
    re | im), a relation dim phases; a triple is scored by the summed moduli of h o exp(i r / q) - t with
    q = rel_embedding_range / pi, and the model always carries its margin (forward = margin - distance). Same
    constructor signature, attribute names, state_dict keys and initialisation order as the reference (two nn.Embedding
    tables, then the entity and the relation uniform init), so a seeded construction gives the reference's tables.
    Distances and training run in the HIP kernels (rotate.hip); there is no tensor-level _calc."""

    native_model = _native.PT_ROTATE

    def __init__(self, ent_tot, rel_tot, dim=100, margin=6.0, epsilon=2.0):
        super(RotatE, self).__init__(ent_tot, rel_tot)
        self.margin = margin
        self.epsilon = epsilon
        self.dim_e = dim * 2
        self.dim_r = dim
        self.ent_embeddings = self._embedding(self.ent_tot, self.dim_e)
        self.rel_embeddings = self._embedding(self.rel_tot, self.dim_r)
        self.ent_embedding_range = nn.Parameter(torch.Tensor([(self.margin + self.epsilon) / self.dim_e]),
                                                requires_grad=False)
        self._uniform_(self.ent_embeddings.weight.data, -self.ent_embedding_range.item(),
                       self.ent_embedding_range.item())
        self.rel_embedding_range = nn.Parameter(torch.Tensor([(self.margin + self.epsilon) / self.dim_r]),
                                                requires_grad=False)
        self._uniform_(self.rel_embeddings.weight.data, -self.rel_embedding_range.item(),
                       self.rel_embedding_range.item())
        self.margin = nn.Parameter(torch.Tensor([margin]))
        self.margin.requires_grad = False
        self.margin_flag = True   # (what Trainer reads: the loss is handed margin - distance)

    def phase_divisor(self):
        """q of phase = r / q, formed as the reference forms it (RotatE.py:51): a Python double divided by the float32
        pi_const tensor, on the CPU whatever device the model is on."""
        return float((self.rel_embedding_range.item() / self.pi_const.detach().cpu()).item())

    def native_desc(self, opt=_native.PT_SGD, lr=0.0, margin=0.0, accs=(None, None, None)):
        ent, rel = self.ent_embeddings.weight, self.rel_embeddings.weight
        if ent.shape[1] != 2 * rel.shape[1]:
            raise RuntimeError("RotatE tables must be [ent_tot][2 * dim] and [rel_tot][dim]")
        for t in (ent, rel):
            if not t.is_cuda:
                raise RuntimeError("model tables are on %s: call model.cuda() first (the MI355X build has no "
                                   "CPU path)" % t.device)
            if t.dtype != torch.float32 or not t.is_contiguous():
                raise RuntimeError("model tables must be contiguous float32")
        d = _native.ModelDesc()
        d.model = self.native_model
        d.p_norm, d.norm_flag = 1, 0   # (fields the RotatE kernels do not read)
        d.opt = opt
        d.lr = float(lr)
        d.margin = float(margin)
        d.ent_total = ent.shape[0]
        d.rel_total = rel.shape[0]
        d.dim = rel.shape[1]
        d.ent = ent.data_ptr()
        d.rel = rel.data_ptr()
        ea, ra = accs[:2]
        d.ent_acc = ea.data_ptr() if ea is not None else None
        d.rel_acc = ra.data_ptr() if ra is not None else None
        d.phase_div = self.phase_divisor()
        return d

    def forward(self, data):
        return self.margin - self.native_score(data)

    def regularization(self, data):
        raise NotImplementedError("regularisation is outside the accelerated path (regul_rate is 0 in every config)")

    def predict(self, data):
        score = -self.forward(data)
        return score.cpu().data.numpy()
