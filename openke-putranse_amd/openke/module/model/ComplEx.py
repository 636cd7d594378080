import torch

from ... import _native
from .Model import Model


class ComplEx(Model):
    """ComplEx (openke/module/model/ComplEx.py:5-62): every entity and relation is a complex vector kept as two real
    tables, a triple is scored by s = sum_j h_re t_re r_re + h_im t_im r_re + h_re t_im r_im - h_im t_re r_im (the real
    part of <h o r, conj(t)>), higher is better; forward returns the score, predict its negative. Same constructor
    signature, attribute names, state_dict keys and initialisation order as the reference (four nn.Embedding tables -
    ent_re, ent_im, rel_re, rel_im - then xavier on the four in that order), so a seeded construction gives the
    reference's tables. Scores and training run in the HIP kernels (complex.hip); there is no tensor-level _calc. The
    forward ignores data['mode'] as the reference's does: head_batch / tail_batch work in predict, where one fixed row
    and one relation row broadcast against the varying rows, and training takes normal sampling only. The regulariser
    is computed inside the native step (NegativeSampling(regul_rate=)); regularization() returns the reference's value
    from the tables. The reference defines no l3_regularization."""

    native_model = _native.PT_COMPLEX
    p_norm, norm_flag = 1, False   # (fields of the native descriptor the ComplEx kernels do not read)

    def __init__(self, ent_tot, rel_tot, dim=100):
        super(ComplEx, self).__init__(ent_tot, rel_tot)
        self.dim = dim
        self.ent_re_embeddings = self._embedding(self.ent_tot, self.dim)
        self.ent_im_embeddings = self._embedding(self.ent_tot, self.dim)
        self.rel_re_embeddings = self._embedding(self.rel_tot, self.dim)
        self.rel_im_embeddings = self._embedding(self.rel_tot, self.dim)
        self._xavier_uniform_(self.ent_re_embeddings.weight.data)
        self._xavier_uniform_(self.ent_im_embeddings.weight.data)
        self._xavier_uniform_(self.rel_re_embeddings.weight.data)
        self._xavier_uniform_(self.rel_im_embeddings.weight.data)

    # what the shared plumbing (Model.native_score, Trainer, Tester) asks an entity / relation table for - device, row
    # count, dim: the re tables (not parameters of their own: state_dict has the reference's four keys only)
    @property
    def ent_embeddings(self):
        return self.ent_re_embeddings

    @property
    def rel_embeddings(self):
        return self.rel_re_embeddings

    def tables(self):
        """(ent_re, rel_re, None, ent_im, rel_im) weight tensors: the im tables ride the native descriptor's
        ent_transfer / rel_transfer fields."""
        return (self.ent_re_embeddings.weight, self.rel_re_embeddings.weight, None, self.ent_im_embeddings.weight,
                self.rel_im_embeddings.weight)

    def native_desc(self, opt=_native.PT_SGD, lr=0.0, margin=0.0, accs=(None, None, None)):
        ent_re, rel_re, _, ent_im, rel_im = self.tables()
        if ent_re.shape != ent_im.shape or rel_re.shape != rel_im.shape or ent_re.shape[1] != rel_re.shape[1]:
            raise RuntimeError("ComplEx: the re and im tables of a pair must have equal shapes, and all four one dim")
        return super(ComplEx, self).native_desc(opt, lr, margin, accs)

    def forward(self, data):
        return -self.native_score(data)

    def _rows(self, data):
        dev = self.ent_re_embeddings.weight.device
        h, t, r = (self._ids(data[k], dev) for k in ('batch_h', 'batch_t', 'batch_r'))
        return (self.ent_re_embeddings(h), self.ent_im_embeddings(h), self.ent_re_embeddings(t),
                self.ent_im_embeddings(t), self.rel_re_embeddings(r), self.rel_im_embeddings(r))

    def regularization(self, data):
        return sum(torch.mean(x ** 2) for x in self._rows(data)) / 6

    def predict(self, data):
        score = -self.forward(data)
        return score.cpu().data.numpy()
