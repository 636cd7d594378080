import torch
import torch.nn as nn
import torch.nn.functional as F

from .Loss import Loss


class SoftplusLoss(Loss):
    """(mean(softplus(-p)) + mean(sum_k w_k softplus(n_k))) / 2 with w = softmax(n * adv_temperature) over a
    positive's negatives, detached, or 1 / K without a temperature (openke/module/loss/SoftplusLoss.py:22-26).
    softplus(x) = -logsigmoid(-x), so this is SigmoidLoss's function; nn.Softplus's threshold at 20 moves the value by
    at most exp(-20) = 2e-9. In training the value and its gradient are computed inside the HIP step as SigmoidLoss's
    (k_step_distmult: Trainer accepts this loss for DistMult); forward() here evaluates the reference's expression on
    given score tensors (value only)."""

    def __init__(self, adv_temperature=None):
        super(SoftplusLoss, self).__init__()
        self.criterion = nn.Softplus()
        if adv_temperature is not None:
            self.adv_temperature = nn.Parameter(torch.Tensor([adv_temperature]))
            self.adv_temperature.requires_grad = False
            self.adv_flag = True
        else:
            self.adv_flag = False

    def get_weights(self, n_score):
        return F.softmax(n_score * self.adv_temperature, dim=-1).detach()

    def forward(self, p_score, n_score):
        if self.adv_flag:
            return (self.criterion(-p_score).mean() +
                    (self.get_weights(n_score) * self.criterion(n_score)).sum(dim=-1).mean()) / 2
        return (self.criterion(-p_score).mean() + self.criterion(n_score).mean()) / 2

    def predict(self, p_score, n_score):
        score = self.forward(p_score, n_score)
        return score.cpu().data.numpy()
