"""PQ_Transformer: joint 3-D object (box) and layout (quad) prediction on a point cloud.

Same constructor, `forward(inputs: dict) -> end_points: dict` contract, `end_points` keys and
`state_dict` names as the reference's models/pq_transformer.py:123-278.  Data flow (:196-267):

    backbone (4 SA + 2 FP)            -> 1024 seeds x 288 ch
    FPSModule(256) on the seeds       -> quad queries
    VotingModule + L2-normalise + SA  -> 256 object queries
    proposal heads on both query sets -> initial centres (used as query positions)
    6 x TransformerDecoderLayer over the 512 joint queries, keys = projected seed features,
        each followed by an object head and a quad head ("0head_".."4head_", "last_")

The heads themselves -- modules, stacks, decode, grouped backward and every switch of theirs -- are models/pred_heads.py; this
module holds the model and asks it for one object per forward pass (pred_heads.begin).
"""
import os
import sys

import torch
from torch import nn

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
for _p in (_HERE, _ROOT, os.path.join(_ROOT, "pointnet2")):
    if _p not in sys.path:
        sys.path.append(_p)

from backbone_module import Pointnet2Backbone, new_step_stream  # noqa: E402
from transformer import TransformerDecoderLayer  # noqa: E402
import transformer as transformer_mod  # noqa: E402
import decoder_rows  # noqa: E402
from utils.pointnet_util import FPSModule  # noqa: E402
from utils import fused_attention  # noqa: E402
from pointnet2_modules import PointnetSAModuleVotes  # noqa: E402
from voting_module import VotingModule  # noqa: E402
import rows_f32  # noqa: E402
import rows_mlp  # noqa: E402
import sa_fused  # noqa: E402
from sa_fused import E16  # noqa: E402
import pred_heads  # noqa: E402
# (functions and classes only: a switch of the heads exists in pred_heads alone, a copy here would be dead)
from pred_heads import PredictHead, QuadPredictHead, seat_head_parameters, rows, lin, conv1x1, conv1x1_pair  # noqa: E402,F401

# "capture": overlap the decoder's key sides on a side stream while a hipGraph is being captured (in eager mode the
# extra stream switches cost more host time than the overlap returns); tests set "always" / "inline"
_OVERLAP_KEY_SIDE = "capture"
_SEED_FANOUT = True         # the seed features' three consumers behind one n-ary gradient add (decoder_rows.FanOut)
_KEY_SIDE_EARLY = True      # fork the key sides right behind the backbone (see PQ_Transformer._forward)
_WGRAD_SIDE = True
# The early weight-gradient flush runs on a stream of its own ("own"; "sampling" = behind the next batch's sampling chain on
# the backbone's side stream, as until the end of round 3: 10.77 vs 10.69 ms).  More flush points, in front of decoder layers,
# were measured and lost: one 11.04 ms, two 13.6, five 15.0 -- every fork / join pair inside the captured step costs more
# than the overlap returns.
_FLUSH_STREAM = "own"
# The decoder's entry: the two query projections become the first layer's joint f32 rows and their 16-bit twin in one launch
# (decoder_rows.JoinRows; backward one launch too) instead of torch.cat of two channel-major views, a transposing copy and a
# cast, and the casts and the f32 add of their way back.  False: the concatenation, as before -- the same bits.
_JOIN_ROWS = True


class PositionEmbeddingLearned(nn.Module):
    """xyz (B,P,C_in) -> learned embedding (B,288,P): Conv1d, BN, ReLU, Conv1d (reference :17-33)."""

    def __init__(self, input_channel, num_pos_feats=288):
        super().__init__()
        self.position_embedding_head = nn.Sequential(
            nn.Conv1d(input_channel, num_pos_feats, kernel_size=1),
            nn.BatchNorm1d(num_pos_feats),
            nn.ReLU(inplace=True),
            nn.Conv1d(num_pos_feats, num_pos_feats, kernel_size=1))

    def forward(self, xyz):
        head = self.position_embedding_head
        B, P, _ = xyz.shape
        x = getattr(xyz, "omnipq_rows2d", None)      # the same positions embedded by several layers (the decoder's
        if x is None or x.shape != (B * P, xyz.shape[2]):   # key side): one row view, so rows_mlp prepares it once
            x = xyz.reshape(B * P, -1)
            if not xyz.requires_grad:
                xyz.omnipq_rows2d = x
        stack = [rows_mlp.Layer(head[0].weight, head[0].bias, head[1]), rows_mlp.Layer(head[3].weight, head[3].bias)]
        if rows_mlp.usable(x, stack, self.training):
            x = rows_mlp.run(x, stack, self.training, eval_chain=True)
        else:
            x = lin(rows_f32.bn_act(lin(x, head[0]), head[1]), head[3])
        return x.view(B, P, -1).transpose(1, 2)


class PQ_Transformer(nn.Module):
    def __init__(self, input_feature_dim, num_class, num_proposal, num_quad_proposal, num_heading_bin,
                 num_size_cluster, mean_size_arr, sampling='vote', num_layer=6, aux_loss=False,
                 decoder_num=1, args=None):
        super().__init__()
        self.i = 0
        self.input_feature_dim = input_feature_dim
        self.num_proposal = num_proposal
        self.num_class = num_class
        self.num_size_cluster = num_size_cluster
        self.mean_size_arr = mean_size_arr
        self.num_heading_bin = num_heading_bin
        self.aux_loss = aux_loss
        self.sampling = sampling
        self.num_quad_proposal = num_quad_proposal
        self.num_layer = num_layer
        self.decoder_num = decoder_num

        self.backbone = Pointnet2Backbone(input_feature_dim=input_feature_dim)
        hidden_dim = 288
        self.decoder_key_proj = nn.Conv1d(288, hidden_dim, kernel_size=1)
        self.decoder_query_proj = nn.Conv1d(288, hidden_dim, kernel_size=1)
        self.quad_decoder_query_proj = nn.Conv1d(288, hidden_dim, kernel_size=1)
        self.fps_module = FPSModule(self.num_quad_proposal)
        # the seeds are the sa2 centres (fp2_xyz): their sampling is coordinate-only, let the plan do it
        self.backbone.plan_extra = {"sa2": self.num_quad_proposal}
        if self.sampling != 'vote':
            raise NotImplementedError
        self.vote = VotingModule(1, 288)
        self.vote_aggregation = PointnetSAModuleVotes(npoint=self.num_proposal, radius=0.3, nsample=16,
                                                      mlp=[288, 288, 288, 288], use_xyz=True,
                                                      normalize_xyz=True)
        self.vote_aggregation.omnipq_stage = "vote"
        self.quad_proposal = QuadPredictHead(hidden_dim)
        self.proposal = PredictHead(hidden_dim, num_heading_bin, num_size_cluster, num_class, mean_size_arr)

        self.prediction_heads = nn.ModuleList()
        self.prediction_quad_heads = nn.ModuleList()
        self.decoder = nn.ModuleList()
        self.decoder_self_posembeds = nn.ModuleList()
        self.decoder_cross_posembeds = nn.ModuleList()
        for i in range(6):      # six layers are always built; num_layer of them run (:180-190)
            self.prediction_heads.append(
                PredictHead(hidden_dim, num_heading_bin, num_size_cluster, num_class, mean_size_arr))
            self.prediction_quad_heads.append(QuadPredictHead(hidden_dim))
            self.decoder_cross_posembeds.append(PositionEmbeddingLearned(3, 288))
            self.decoder_self_posembeds.append(PositionEmbeddingLearned(3, 288))
            self.decoder.append(TransformerDecoderLayer(
                self_posembed=self.decoder_self_posembeds[i],
                cross_posembed=self.decoder_cross_posembeds[i]))

        self.init_weights()
        self.init_bn_momentum()
        nn.SyncBatchNorm.convert_sync_batchnorm(self)      # in place for every child BN (:194)

    def forward(self, inputs):
        E16.autocast()                 # bf16 / fp16 autocast: the hand-written kernels' element type for this step
        arena = sa_fused.arena_of(self)
        with sa_fused.deferred_counters(), arena.step(inputs['point_clouds'].device):
            return self._forward(inputs)

    def _forward(self, inputs):
        if self.training and inputs['point_clouds'].is_cuda:
            fused_attention.STATE.advance(inputs['point_clouds'].device)     # new dropout masks this step
        end_points = self.backbone(inputs['point_clouds'], {})
        seed_xyz = end_points['fp2_xyz']
        seed_features = end_points['fp2_features']
        if _WGRAD_SIDE and seed_features.is_cuda and seed_features.requires_grad:
            # backward: when the gradient reaches this point the decoder, the heads and the voting module are done --
            # their collected weight gradients (sa_fused.deferred_wgrads) start on a side stream underneath the
            # backbone's backward pass
            twin = getattr(seed_features, "omnipq_rows16", None)
            seed_features = sa_fused.WgradFlushPoint.apply(
                seed_features, lambda dev=seed_features.device: self._flush_stream(dev))
            if twin is not None:
                seed_features.omnipq_rows16 = twin
        # three consumers (layout branch, voting, the decoder's memory): their gradients -- (B, C, K) views of position-major
        # rows -- meet in ONE n-ary add (decoder_rows.FanOut) instead of autograd's two strided adds
        sf_quad = sf_vote = sf_key = seed_features
        if _SEED_FANOUT and seed_features.is_cuda and seed_features.requires_grad and torch.is_grad_enabled():
            twin = getattr(seed_features, "omnipq_rows16", None)
            sf_quad, sf_vote, sf_key = decoder_rows.FanOut.apply(seed_features, 3)
            if twin is not None:
                sf_quad.omnipq_rows16 = sf_vote.omnipq_rows16 = sf_key.omnipq_rows16 = twin

        # The decoder's memory and the six layers' key / value sides depend on the seeds only: with _KEY_SIDE_EARLY their
        # side-stream chain (~30 launches) forks HERE, underneath the voting module, the vote aggregation (whose sampling is
        # 256 dependent rounds on eight CUs) and the proposal heads, instead of underneath the first decoder layers.
        key = key_sides = None
        key_pos = seed_xyz
        overlap = _OVERLAP_KEY_SIDE == "always" or \
            (_OVERLAP_KEY_SIDE == "capture" and seed_features.is_cuda and torch.cuda.is_current_stream_capturing())
        if _KEY_SIDE_EARLY and overlap and transformer_mod._USE_ROWS:
            key = conv1x1(sf_key, self.decoder_key_proj)
            if all(decoder_rows.usable(layer, key, key) for layer in self.decoder):
                key_sides = decoder_rows.precompute_key_sides(list(self.decoder), key, key_pos)

        # layout branch: FPS over the seeds
        quad_xyz, quad_feature, _ = self.fps_module(seed_xyz, sf_quad, self.backbone.take_extra("sa2"))
        end_points['aggregated_sample_xyz'] = quad_xyz

        # object branch: vote, normalise, aggregate
        # vote + the reference's L2 normalisation over the channels (:216-217), fused on the row kernels
        vote_xyz, vote_features = self.vote(seed_xyz, sf_vote, normalized=True)
        end_points['vote_xyz'] = vote_xyz
        end_points['vote_features'] = vote_features
        cluster_xyz, cluster_feature, _ = self.vote_aggregation(vote_xyz, vote_features)
        end_points['aggregated_vote_xyz'] = cluster_xyz
        end_points['cluster_feature'] = cluster_feature

        # the heads of this forward pass: where the base positions' gradient goes and how the stages' backward runs
        heads = pred_heads.begin(cluster_xyz, cluster_feature, self.num_layer + 1, self.training)
        cluster_feature = heads.feature

        center, center_q, end_points, pos_joint = heads.stage(
            self.proposal, self.quad_proposal, cluster_feature, quad_feature, cluster_xyz, quad_xyz, end_points,
            'proposal_', want_pos=True)
        # the reference clones here (:236-237); nothing writes into these tensors afterwards, a detached alias suffices
        base_xyz = center.detach()
        base_xyz_q = center_q.detach()

        query_obj, query_quad = conv1x1_pair(cluster_feature, self.decoder_query_proj,
                                             quad_feature, self.quad_decoder_query_proj)
        query_joint = None
        if _JOIN_ROWS and transformer_mod._USE_ROWS:
            # the two projections' rows -> the first layer's f32 residual rows and their 16-bit twin, one launch each way
            query_joint = decoder_rows.join_queries(query_obj, query_quad, self.decoder)
        if query_joint is None:
            query_joint = torch.cat((query_obj, query_quad), -1)
        if key is None:
            key = conv1x1(sf_key, self.decoder_key_proj)

        # every layer attends to the same memory: their key/value sides run ahead on a side stream
        if key_sides is None:
            key_sides = [None] * self.num_layer
            if overlap and transformer_mod._USE_ROWS and \
                    all(decoder_rows.usable(layer, query_joint, key) for layer in self.decoder):
                key_sides = decoder_rows.precompute_key_sides(list(self.decoder), key, key_pos)

        for i in range(self.num_layer):
            prefix = 'last_' if (i == self.num_layer - 1) else f'{i}head_'
            # (the pair decode of the stage before leaves both centres side by side already)
            query_pos_joint = pos_joint if pos_joint is not None else torch.cat([base_xyz, base_xyz_q], 1)
            pos_joint = None
            query_joint = self.decoder[i](query_joint, key, query_pos_joint, key_pos, key_sides[i], self.num_proposal)
            n_obj, n_quad = self.num_proposal, query_joint.shape[2] - self.num_proposal
            query, query_q = torch.split(query_joint, [n_obj, n_quad], dim=2)     # one cat in backward
            rows16 = getattr(query_joint, 'omnipq_rows16', None)          # (B, P, C) bf16 twin from the row-major decoder
            rows_obj = rows_quad = None
            blocks = getattr(query_joint, 'omnipq_rows_split', None)
            if blocks is not None:
                # the layer's last LayerNorm wrote the two heads' row blocks itself, and its backward takes their gradients
                # next to the joint rows' (decoder_rows.LN_SPLIT)
                rows_obj, rows_quad = blocks
            elif decoder_rows.split_usable(rows16):
                # the two heads' inputs as contiguous row blocks, and the joint rows' three gradients (two heads, next
                # layer) merged by one launch in backward
                rows_obj, rows_quad, alias = decoder_rows.SplitRows.apply(rows16, n_obj)
                rows_obj, rows_quad = rows_obj.view(-1, n_obj, rows16.shape[2]), rows_quad.view(-1, n_quad, rows16.shape[2])
                query_joint.omnipq_rows16 = alias
            elif rows16 is not None:
                rows_obj, rows_quad = torch.split(rows16, [n_obj, n_quad], dim=1)
            base_xyz, base_xyz_q, end_points, pos_joint = heads.stage(
                self.prediction_heads[i], self.prediction_quad_heads[i], query, query_q, cluster_xyz, quad_xyz,
                end_points, prefix, rows_obj, rows_quad, want_pos=i + 1 < self.num_layer)
            base_xyz = base_xyz.detach()
            base_xyz_q = base_xyz_q.detach()
        heads.finish(end_points)
        return end_points

    def __getstate__(self):
        state = self.__dict__.copy()
        state.pop("_omnipq_flush_streams", None)        # streams do not travel with a copy of the module (EMA teacher, torch.save)
        return state

    def _flush_stream(self, device):
        """The stream early weight-gradient flushes run on (sa_fused.WgradFlushPoint)."""
        if _FLUSH_STREAM == "sampling":
            return self.backbone._side_stream(device)
        streams = self.__dict__.setdefault("_omnipq_flush_streams", {})
        if device not in streams:
            streams[device] = new_step_stream(device, owner=self)
        return streams[device]

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        with torch.no_grad():
            for m in self.modules():
                if isinstance(m, (PredictHead, QuadPredictHead)):
                    seat_head_parameters(m)
        return out

    def prefetch(self, inputs, trusted=False, at_next_forward=False, footprint=None, resume=False):
        """Optional: start the coordinate-only sampling (FPS chain of the backbone) of a FUTURE batch on
        a side stream; `forward` on the same `inputs['point_clouds']` tensor then skips it.  Results do
        not change (sa1's FPS depends only on the input cloud).  at_next_forward: start it inside the
        next forward() call (of the CURRENT batch) instead of now, see Pointnet2Backbone.prefetch.  resume: continue the
        sa1 level where prefetch_head() of this batch stopped."""
        self.backbone.prefetch(inputs['point_clouds'], trusted, at_next_forward, footprint, resume)

    def prefetch_head(self, inputs, rounds, trusted=False, footprint="small"):
        """Optional: the first `rounds` rounds of the sa1 sampling of a batch TWO steps ahead, on a second side stream
        (Pointnet2Backbone.prefetch_head); `prefetch(..., resume=True)` of that batch continues from there."""
        self.backbone.prefetch_head(inputs['point_clouds'], rounds, trusted, footprint)

    def hand_over_head(self):
        """Make the sampled head the state the next resumed chain continues (Pointnet2Backbone.hand_over_head)."""
        self.backbone.hand_over_head()

    def forget_prefetch(self):
        """Forget the host-side record of a sampling plan in flight (Pointnet2Backbone.forget_plan)."""
        self.backbone.forget_plan()

    def join_prefetch(self):
        """Order the current stream after the sampling stream (needed before a graph capture ends)."""
        self.backbone.join()

    def init_weights(self):
        for p in self.decoder.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    def init_bn_momentum(self):
        for m in self.modules():
            if isinstance(m, (nn.BatchNorm2d, nn.BatchNorm1d)):
                m.momentum = 0.1
