"""`paddle3d.models.classification.paconv` on the device op (paddle3d_amd/ops/assign_score_withk.py): PAConv's
ModelNet40 classifier (paconv.py) and its ScoreNet (score_net.py).

ScoreNet(in_channel, out_channel, hidden_unit=[16], last_bn=False)
    score_net.py: 1x1 Conv2d / BN / ReLU over the (neighbour - centre, neighbour) input, a last 1x1 Conv2d, softmax
    (or sigmoid) over the weight banks + bias_attr -> scores [B, N, K, M].
PAConv(k_neighbors=20, calc_scores='softmax', num_matrices=(8, 8, 8, 8), dropout=0.5)
    knn (torch matmul + topk, as the reference), get_scorenet_input, feat_trans_dgcnn, four assign_score_withk layers
    with BN / ReLU, conv5, the max + avg pooled head.  forward({'data': [B, N, 3], 'labels': [B]}) returns
    {'loss': ...} in training mode and {'preds': [B, 40]} in eval mode.

Parameter names are the reference's (matrice1..4, scorenet1..4.mlp_convs_hidden.*, bn*, conv5, linear*), so
checkpoint.load_paddle_state_dict loads a Paddle checkpoint without a name table.  `self.assign_score_withk` is an
attribute, as in the reference: the op (GPU only) can be swapped for another formulation.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F
from torch import nn

from .ops.assign_score_withk import assign_score_withk

__all__ = ["ScoreNet", "PAConv"]


class ScoreNet(nn.Module):
    def __init__(self, in_channel, out_channel, hidden_unit=(16,), last_bn=False):
        super().__init__()
        self.hidden_unit = list(hidden_unit) if hidden_unit else []
        self.last_bn = last_bn
        self.mlp_convs_hidden = nn.ModuleList()
        self.mlp_bns_hidden = nn.ModuleList()
        if not self.hidden_unit:
            self.mlp_convs_nohidden = nn.Conv2d(in_channel, out_channel, 1, bias=not last_bn)
            if last_bn:
                self.mlp_bns_nohidden = nn.BatchNorm2d(out_channel)
        else:
            widths = [in_channel] + self.hidden_unit
            for i in range(len(self.hidden_unit)):
                self.mlp_convs_hidden.append(nn.Conv2d(widths[i], widths[i + 1], 1, bias=False))
                self.mlp_bns_hidden.append(nn.BatchNorm2d(widths[i + 1]))
            self.mlp_convs_hidden.append(nn.Conv2d(self.hidden_unit[-1], out_channel, 1, bias=not last_bn))
            self.mlp_bns_hidden.append(nn.BatchNorm2d(out_channel))

    def forward(self, xyz, calc_scores="softmax", bias_attr=0):
        scores = xyz
        if not self.hidden_unit:
            scores = self.mlp_convs_nohidden(scores)
            if self.last_bn:
                scores = self.mlp_bns_nohidden(scores)
        else:
            last = len(self.mlp_convs_hidden) - 1
            for i, conv in enumerate(self.mlp_convs_hidden):
                if i == last:
                    scores = self.mlp_bns_hidden[i](conv(scores)) if self.last_bn else conv(scores)
                else:
                    scores = F.relu(self.mlp_bns_hidden[i](conv(scores)))
        if calc_scores == "softmax":
            scores = F.softmax(scores, dim=1) + bias_attr  # B, m, N, K
        elif calc_scores == "sigmoid":
            scores = torch.sigmoid(scores) + bias_attr
        else:
            raise ValueError("Not Implemented!")
        return scores.permute(0, 2, 3, 1)  # B, N, K, m


class PAConv(nn.Module):
    def __init__(self, k_neighbors=20, calc_scores="softmax", num_matrices=(8, 8, 8, 8), dropout=0.5):
        super().__init__()
        if calc_scores not in ("softmax", "sigmoid"):
            raise ValueError(f"Unsupported calc scores type {calc_scores}")
        self.k = k_neighbors
        self.calc_scores = calc_scores
        self.assign_score_withk = assign_score_withk
        self.m1, self.m2, self.m3, self.m4 = num_matrices
        self.scorenet1 = ScoreNet(6, self.m1, hidden_unit=[16])
        self.scorenet2 = ScoreNet(6, self.m2, hidden_unit=[16])
        self.scorenet3 = ScoreNet(6, self.m3, hidden_unit=[16])
        self.scorenet4 = ScoreNet(6, self.m4, hidden_unit=[16])
        i1, o1, o2, o3, o4 = 3, 64, 64, 128, 256
        for name, m, cin, cout in (("matrice1", self.m1, i1, o1), ("matrice2", self.m2, o1, o2),
                                   ("matrice3", self.m3, o2, o3), ("matrice4", self.m4, o3, o4)):
            # kaiming_normal_init(relu) of [m, 2cin, cout] (fan_in = 2cin * cout), laid out [2cin, m * cout]
            w = torch.randn(m, cin * 2, cout) * (2.0 / (cin * 2 * cout)) ** 0.5
            self.register_parameter(name, nn.Parameter(w.permute(1, 0, 2).reshape(cin * 2, m * cout).contiguous()))
        self.bn1, self.bn2, self.bn3, self.bn4 = (nn.BatchNorm1d(c) for c in (o1, o2, o3, o4))
        self.bn5 = nn.BatchNorm1d(1024)
        self.conv5 = nn.Sequential(nn.Conv1d(512, 1024, kernel_size=1, bias=False), self.bn5)
        self.linear1 = nn.Linear(2048, 512, bias=False)
        self.bn11 = nn.BatchNorm1d(512)
        self.dp1 = nn.Dropout(p=dropout)
        self.linear2 = nn.Linear(512, 256, bias=False)
        self.bn22 = nn.BatchNorm1d(256)
        self.dp2 = nn.Dropout(p=dropout)
        self.linear3 = nn.Linear(256, 40)
        for mod in self.modules():
            if isinstance(mod, (nn.Linear, nn.Conv1d, nn.Conv2d)):
                nn.init.kaiming_normal_(mod.weight)
                if mod.bias is not None:
                    nn.init.zeros_(mod.bias)

    def knn(self, x, k):
        inner = -2 * torch.matmul(x.transpose(1, 2), x)
        xx = torch.sum(x ** 2, dim=1, keepdim=True)
        pairwise_distance = -xx - inner - xx.transpose(1, 2)
        idx = pairwise_distance.topk(k=k, dim=-1)[1]  # B, N, k
        return idx, pairwise_distance

    def get_scorenet_input(self, x, idx, k):
        """(neighbour - centre, neighbour) -> [B, 6, N, k]."""
        B, N = x.shape[0], x.shape[2]
        x = x.reshape(B, -1, N)
        idx = (idx + torch.arange(B, device=x.device).reshape(-1, 1, 1) * N).reshape(-1)
        C = x.shape[1]
        x = x.transpose(1, 2)
        neighbor = x.reshape(B * N, -1)[idx].reshape(B, N, k, C)
        x = x.reshape(B, N, 1, C).expand(B, N, k, C)
        return torch.cat((neighbor - x, neighbor), dim=3).permute(0, 3, 1, 2)

    def feat_trans_dgcnn(self, point_input, kernel, m):
        """(point_output, center_output) [B, N, m, cout]."""
        B, _, N = point_input.shape
        xt = point_input.transpose(1, 2)
        point_output = torch.matmul(xt.repeat(1, 1, 2), kernel).reshape(B, N, m, -1)
        center_output = torch.matmul(xt, kernel[:point_input.shape[1]]).reshape(B, N, m, -1)
        return point_output, center_output

    def get_loss(self, pred, label):
        label = label.reshape(-1)
        eps = 0.2
        n_class = pred.shape[1]
        one_hot = F.one_hot(label.long(), n_class).to(pred.dtype)
        one_hot = one_hot * (1 - eps) + (1 - one_hot) * eps / (n_class - 1)
        log_prb = F.log_softmax(pred, dim=1)
        return {"loss": -(one_hot * log_prb).sum(dim=1).mean()}

    def _layer(self, feats, xyz, idx, kernel, m, scorenet, bn):
        point, center = self.feat_trans_dgcnn(point_input=feats, kernel=kernel, m=m)
        score = scorenet(xyz, calc_scores=self.calc_scores, bias_attr=0.5)
        point = self.assign_score_withk(scores=score, points=point, centers=center, knn_idx=idx)
        return F.relu(bn(point))

    def forward(self, inputs):
        x = inputs["data"].transpose(1, 2)  # B, 3, N
        B = x.shape[0]
        idx, _ = self.knn(x, k=self.k)
        xyz = self.get_scorenet_input(x, idx=idx, k=self.k)
        point1 = self._layer(x, xyz, idx, self.matrice1, self.m1, self.scorenet1, self.bn1)
        point2 = self._layer(point1, xyz, idx, self.matrice2, self.m2, self.scorenet2, self.bn2)
        point3 = self._layer(point2, xyz, idx, self.matrice3, self.m3, self.scorenet3, self.bn3)
        point4 = self._layer(point3, xyz, idx, self.matrice4, self.m4, self.scorenet4, self.bn4)
        point = torch.cat((point1, point2, point3, point4), dim=1)
        point = F.relu(self.conv5(point))
        point11 = F.adaptive_max_pool1d(point, 1).reshape(B, -1)
        point22 = F.adaptive_avg_pool1d(point, 1).reshape(B, -1)
        point = torch.cat((point11, point22), 1)
        point = self.dp1(F.relu(self.bn11(self.linear1(point))))
        point = self.dp2(F.relu(self.bn22(self.linear2(point))))
        point = self.linear3(point)
        if self.training:
            return self.get_loss(point, inputs["labels"])
        return {"preds": point}
