"""MI355X-native mirror of the retrieval path of ``modules/clip4clip.py`` (meanP / loose_type):
CLIP4Clip.from_pretrained (local checkpoint), forward, get_sequence_output, get_visual_output,
get_similarity_logits, _loose_similarity, get_video_mask_after_cluster - same signatures and return conventions
(SURVEY.md §8b, rows S1/S2).  All compute goes through ``torch.ops.centerclip.*``.

Training mode returns the reference's loss (feature all-gather -> logits -> symmetric CrossEn, clip4clip.py:245-262),
differentiable with respect to the features and logit_scale; the towers have no backward (encoder backward,
DDP gradient all-reduce and the optimiser are out of scope).
sim_header 'seqTransf' (clip4clip.py:335-349): frame_position_embeddings + transformerClip under the reference's names,
applied to the per-segment features before the pooling (eval: cc_seqtransf_forward_f32 in one enqueue; training: the blocks'
HIP forward / backward with the key mask, centerclip_amd.train.seq_head_train).
Not built: tightTransf / seqLSTM (the reference cannot run them either), weight download.
"""
import torch
from torch import nn

from . import _lib as L
from . import ops
from . import torch_ops as T
from .clip import Transformer, _Pack, build_clip_model, load_clip_state_dict, zero_scalar
from . import dist as ccdist
from .dist import AllGather, PackedAllGather, all_gather
from .losses import contrastive_loss


class CLIP4Clip(nn.Module):
    def __init__(self, clip_state_dict, task_config):
        super().__init__()
        self.task_config = task_config
        self.loose_type = bool(getattr(task_config, "loose_type", True))
        self.linear_patch = getattr(task_config, "linear_patch", '2d')
        self.sim_header = getattr(task_config, "sim_header", 'meanP')
        if self.linear_patch not in ('2d', '3d'):
            raise ValueError("linear_patch must be '2d' or '3d'")
        if self.sim_header not in ("meanP", "seqTransf") or not self.loose_type:
            # (clip4clip.py:332-333,426-427: the reference raises NotImplementedError for seqLSTM and the tight head too)
            raise NotImplementedError("only sim_header 'meanP' and 'seqTransf' with loose_type are built (the reference runs no "
                                      "other head)")
        self.cluster_inter = getattr(task_config, "cluster_inter", 0)
        self.cluster_algo = getattr(task_config, "cluster_algo", None)
        self.deep_cluster = getattr(task_config, "deep_cluster", 0)
        self.video_frames = getattr(task_config, "max_frames", None)
        self.final_frames = task_config.target_frames_blocks[-1]
        self.f_frame_duration = self.video_frames // self.final_frames
        self.pre_visual_pooling = getattr(task_config, "pre_visual_pooling", 0)
        # CAMoE dual softmax (params.py:278; the reference stores the flag and keeps both uses commented out, clip4clip.py:430-432,
        # main.py:526-532): logits S -> S * softmax(S, dim=0) * len(S), in get_similarity_logits, eval_epoch and the training loss
        self.camoe_dsl = bool(getattr(task_config, "camoe_dsl", False))
        self.clip, self.clip_config = build_clip_model(clip_state_dict, convert_fp16=True,
                                                       linear_patch=self.linear_patch, cut_top_layer=0,
                                                       load_state_dict=True, is_eval=False,
                                                       video_frames=self.video_frames, args=task_config,
                                                       quick_gelu=bool(getattr(task_config, "quick_gelu", 1)))
        if self.sim_header == "seqTransf":
            if self.pre_visual_pooling:
                # (the reference would pool first and then index position 512 of the 77-row table)
                raise ValueError("sim_header='seqTransf' needs the per-segment features: pre_visual_pooling is not supported")
            cfg = self.clip_config
            width = cfg['transformer_width']
            if cfg['embed_dim'] != width:
                raise ValueError("sim_header='seqTransf': the head runs on the visual features, so embed_dim (%d) must equal "
                                 "transformer_width (%d)" % (cfg['embed_dim'], width))
            # clip4clip.py:178,187-192: an embedding of context_length rows and module_cross.Transformer (fp32 parameters);
            # the head is CLIP4Clip's own transformer: QuickGELU (module_cross.py) whatever activation the towers use
            self.frame_position_embeddings = nn.Embedding(cfg['context_length'], width)
            self.transformerClip = Transformer(width=width, layers=int(getattr(task_config, "cross_num_hidden_layers", 4)),
                                               heads=cfg['transformer_heads'], quick_gelu=True)
            for blk in self.transformerClip.resblocks:    # nn.MultiheadAttention's own initialisation of the packed in_proj
                nn.init.xavier_uniform_(blk.attn.in_proj_weight)
            self._head_pack = None

    @classmethod
    def from_state_dict(cls, clip_state_dict, task_config):
        """Build from an OpenAI-CLIP style state dict (keys without the 'clip.' prefix).  seqTransf: the head starts from the
        reference's initialisation trick (seq_head_init), as from_pretrained does without a fine-tuned head."""
        model = cls(clip_state_dict, task_config)
        if model.sim_header == "seqTransf":
            with torch.no_grad():
                model.load_state_dict(cls.seq_head_init(clip_state_dict, model.transformerClip.layers), strict=False)
        return model

    def replica(self):
        """A second instance with the same configuration and a copy of the weights, on the same device and in the same mode.
        The fused encoders keep their folded weights and scratch per instance, so two batches can only be in flight at once
        on two instances (eval_epoch(..., in_flight=2): +15 % clips/s - the k-medoids selection and the launch tails of one
        batch run under the other's GEMMs).  Not in the reference (it evaluates one batch at a time)."""
        m = type(self)({k: v.detach() for k, v in self.clip.state_dict().items()}, self.task_config)
        m = m.to(next(self.parameters()).device)
        m.load_state_dict(self.state_dict(), strict=False)
        return m.train(self.training)

    @classmethod
    def from_pretrained(cls, cross_model_name=None, state_dict=None, cache_dir=None, type_vocab_size=2, *inputs,
                        **kwargs):
        """modules/clip4clip.py:27-123 for the built configuration (meanP, linear_patch '2d'): the CLIP weights come
        from <task_config.pretrained_dir>/ViT-B-32.pt (or ViT-B-16.pt), a fine-tuned ``state_dict`` (keys prefixed
        'clip.') overrides them, ``temperature_new`` > 1 replaces logit_scale.  ``cross_model_name`` / ``cache_dir`` /
        ``type_vocab_size`` configure the cross encoder, which only the tightTransf head uses: accepted, unused."""
        task_config = kwargs['task_config']
        if state_dict is None:
            state_dict = {}
        name = getattr(task_config, 'pretrained_clip_name', "ViT-B/32")
        clip_state_dict = load_clip_state_dict(name, pretrained_dir=task_config.pretrained_dir)
        model = cls(clip_state_dict, task_config)
        override = {k[len("clip."):]: v for k, v in state_dict.items() if k.startswith("clip.")}
        if model.linear_patch == '3d' and "visual.conv2.weight" not in override and "visual.conv2.weight" not in clip_state_dict:
            # the reference's initialisation trick (clip4clip.py:46-76): conv2 = conv1 in the centre time slice, zeros around
            w1 = override.get("visual.conv1.weight", clip_state_dict["visual.conv1.weight"]).float()
            w2 = torch.zeros_like(model.clip.visual.conv2.weight)
            w2[:, :, (w2.shape[2] - 1) // 2] = w1
            override["visual.conv2.weight"] = w2
        if override:
            model.clip.load_state_dict(override, strict=False)
        if model.sim_header == "seqTransf":
            head = {k: v for k, v in state_dict.items() if k.startswith(("frame_position_embeddings.", "transformerClip."))}
            if not any(k.startswith("frame_position_embeddings") for k in state_dict):
                head.update(cls.seq_head_init(clip_state_dict, model.transformerClip.layers))
            if head:
                with torch.no_grad():
                    model.load_state_dict(head, strict=False)
        if getattr(task_config, "temperature_new", 0.0) > 1.0:
            with torch.no_grad():                    # (tracked by the packs' version keys, unlike a .data write)
                model.clip.logit_scale.fill_(task_config.temperature_new)
        return model

    @staticmethod
    def seq_head_init(clip_state_dict, layers):
        """The reference's initialisation trick for the seqTransf head (clip4clip.py:97-113), applied when the fine-tuned
        state dict has no frame_position_embeddings: the position rows from CLIP's positional_embedding, block i < layers of
        transformerClip from the text transformer's block i.  -> {name: tensor} under the reference's names."""
        out = {"frame_position_embeddings.weight": clip_state_dict["positional_embedding"].clone()}
        for k, v in clip_state_dict.items():
            if k.startswith("transformer.resblocks.") and int(k.split(".")[2]) < layers:
                out[k.replace("transformer.", "transformerClip.", 1)] = v.clone()
        return out

    # ------------------------------------------------------------------ sim_header 'seqTransf' (clip4clip.py:335-349)
    def _head_weights(self):
        """fp32 position rows + the 12 tensors per block cc_seqtransf_forward_f32 reads (fp16 GEMM weights), rebuilt when a
        parameter's version changes (an in-place write under no_grad is seen; a write through .data needs invalidate())."""
        key = _Pack.signature(self.frame_position_embeddings) + _Pack.signature(self.transformerClip)
        if self._head_pack is None or self._head_pack[0] != key:
            f16 = lambda t: t.detach().to(torch.float16).contiguous()
            f32 = lambda t: t.detach().float().contiguous()
            ws = []
            for blk in self.transformerClip.resblocks:
                ws += [f32(blk.ln_1.weight), f32(blk.ln_1.bias), f16(blk.attn.in_proj_weight), f32(blk.attn.in_proj_bias),
                       f16(blk.attn.out_proj.weight), f32(blk.attn.out_proj.bias), f32(blk.ln_2.weight), f32(blk.ln_2.bias),
                       f16(blk.mlp["c_fc"].weight), f32(blk.mlp["c_fc"].bias), f16(blk.mlp["c_proj"].weight),
                       f32(blk.mlp["c_proj"].bias)]
            self._head_pack = (key, f32(self.frame_position_embeddings.weight), ws)
        return self._head_pack[1], self._head_pack[2]

    def _check_head_input(self, visual_output, video_mask):
        if visual_output.dim() != 3:
            raise ValueError("sim_header='seqTransf' needs the per-segment features [B, T, D]")
        T = visual_output.shape[1]
        if T > self.frame_position_embeddings.num_embeddings:
            raise ValueError("sim_header='seqTransf': %d segments, the frame position table has %d rows"
                             % (T, self.frame_position_embeddings.num_embeddings))
        if tuple(video_mask.shape) != tuple(visual_output.shape[:2]):
            raise ValueError("sim_header='seqTransf': mask %s for features %s" % (tuple(video_mask.shape),
                                                                                 tuple(visual_output.shape)))

    def seq_head(self, visual_output, video_mask):
        """visual_output [B, T, D] + video_mask [B, T] (any strides) -> the head's output [B, T, D] fp32, without gradients
        (clip4clip.py:335-349: + position rows, transformerClip with the key mask, + visual_output).  meanP: the input."""
        if self.sim_header != "seqTransf":
            return visual_output
        self._check_head_input(visual_output, video_mask)
        L.require_device(visual_output, video_mask)
        pos, ws = self._head_weights()
        return torch.ops.centerclip.seqtransf_forward(visual_output.detach().float().contiguous(), video_mask.to(torch.long),
                                                      pos, ws, self.transformerClip.heads)

    def _seq_head_any(self, visual_output, video_mask):
        """The head with gradients when autograd records (training), else seq_head."""
        if self.sim_header != "seqTransf":
            return visual_output
        if torch.is_grad_enabled() and self.training:
            from . import train as cctrain
            self._check_head_input(visual_output, video_mask)
            return cctrain.seq_head_train(self, visual_output, video_mask)
        return self.seq_head(visual_output, video_mask)

    # ------------------------------------------------------------------ forward (clip4clip.py:199-263)
    def forward(self, input_ids=None, token_type_ids=None, attention_mask=None, video=None, video_mask=None,
                pre_visual_pooling=False):
        output_dict = {'sequence_output': None, 'visual_output': None, 'loss': None}
        sequence_output = visual_output = None
        cluster_loss = None
        if input_ids is not None:
            input_ids = input_ids.view(-1, input_ids.shape[-1])
            if attention_mask is not None:
                attention_mask = attention_mask.view(-1, attention_mask.shape[-1])
        if video is not None:
            video = torch.as_tensor(video)
            if video.dtype != torch.uint8:           # uint8 frames go to the patch gather as they are (N3)
                video = video.float()
            b, pair, video_frame = video.shape[:3]
            video = video.reshape((-1,) + tuple(video.shape[3:]))   # [B*T, C, H, W], or [B*T, H, W, C] for uint8 HWC
            video_mask = video_mask.view(-1, video_mask.shape[-1])
            if self.cluster_inter or self.deep_cluster:
                video_mask = self.get_video_mask_after_cluster(video_mask)
        if self.training and torch.is_grad_enabled() and input_ids is not None and video is not None:
            # training (main.py:311): the towers with their backward (centerclip_amd.train), gradients reach every parameter
            from . import train as cctrain
            vfeat, cluster_loss = cctrain.encode_image_train(self.clip, video, video_frame)
            tfeat = cctrain.encode_text_train(self.clip, input_ids)
            sequence_output = tfeat.view(input_ids.size(0), -1, tfeat.size(-1))
            visual_output = vfeat.view(video_mask.size(0), -1, vfeat.size(-1))
        elif input_ids is not None and video is not None:
            # both towers in one enqueue: the text tower's blocks share their launches with the ViT's
            vfeat, tfeat = self.clip.encode_pair(video, input_ids, video_frame=video_frame)
            sequence_output = tfeat.view(input_ids.size(0), -1, tfeat.size(-1))
            visual_output = vfeat.view(video_mask.size(0), -1, vfeat.size(-1))
            cluster_loss = zero_scalar(vfeat.device)
        elif input_ids is not None:
            sequence_output = self.get_sequence_output(input_ids, token_type_ids, attention_mask)
        elif video is not None:
            visual_output, cluster_loss = self.get_visual_output(video, video_mask, video_frame=video_frame)
        output_dict['sequence_output'] = sequence_output
        if video is not None:
            if self.training or not self.pre_visual_pooling:
                output_dict['visual_output'] = visual_output
            else:                                    # clip4clip.py:238-243: normalise, masked mean, normalise
                output_dict['visual_output'] = ops.video_pool_normalize(visual_output, video_mask)
        if self.training:
            # the reference's training branch (clip4clip.py:245-262): features of all ranks -> logits -> symmetric CrossEn.
            # The loss is differentiable with respect to the features and logit_scale (losses.contrastive_loss: forward and
            # gradient in one kernel chain); the features come from the differentiable towers above.
            # seqTransf: the head runs on the local batch, before the exchange (clip4clip.py:340-355)
            seq = sequence_output.contiguous()
            vis = self._seq_head_any(visual_output, video_mask).contiguous()
            vmask = video_mask.contiguous()
            if ccdist.world_size() > 1:              # ONE collective for the three tensors, gradient slices of the own shard back
                vis, vmask, seq = PackedAllGather.apply(vis, vmask, seq)
            # (logit_scale is read on the device: the optimizer changes it every step, and a host copy would be a synchronisation)
            sim_loss, _, _ = contrastive_loss(seq, vis, vmask, self.clip.logit_scale, dsl=self.camoe_dsl)
            output_dict['loss'] = sim_loss + cluster_loss
            output_dict['cluster_loss'] = cluster_loss
            output_dict['sim_loss'] = sim_loss
        return output_dict

    def encode_into(self, sink, input_ids, video, video_mask):
        """The multi-GPU step's producer: forward()'s two towers with the features written straight into a
        dist.PackedFeatures record (sink.vis / sink.seq; the segment mask is copied into sink.mask), so that the exchange
        of clip4clip.py:351-355 is ONE all_gather_into_tensor of preallocated buffers with no packing step."""
        if self.sim_header != "meanP":
            raise NotImplementedError("encode_into: the feature records carry the pooled meanP operands; sim_header=%r runs "
                                      "its head in forward() / get_similarity_logits" % self.sim_header)
        input_ids = input_ids.view(-1, input_ids.shape[-1])
        video = torch.as_tensor(video)
        if video.dtype != torch.uint8:
            video = video.float()
        video_frame = video.shape[2]
        video = video.reshape((-1,) + tuple(video.shape[3:]))
        video_mask = video_mask.view(-1, video_mask.shape[-1])
        if self.cluster_inter or self.deep_cluster:
            video_mask = self.get_video_mask_after_cluster(video_mask)
        self.clip.encode_pair(video, input_ids, video_frame=video_frame, out=(sink.vis, sink.seq))
        sink.mask.copy_(video_mask)
        return sink

    def invalidate(self):
        """After a write through ``.data`` (not version-tracked): drop every cached copy of the parameters."""
        self._ls_key = None
        self._head_pack = None
        self.clip.invalidate()

    def _logit_scale_value(self):
        """Python float of clip.logit_scale, cached per parameter version (no device->host sync per call).  Writes through
        ``.data`` are not seen - use ``with torch.no_grad(): p.fill_()`` or call invalidate()."""
        p = self.clip.logit_scale
        key = (p.data_ptr(), p._version)
        if getattr(self, "_ls_key", None) != key:
            self._ls_key, self._ls_val = key, float(p.detach())
        return self._ls_val

    def get_sequence_output(self, input_ids, token_type_ids=None, attention_mask=None):
        """-> [bs_pair, 1, D] fp32   (clip4clip.py:265-272)"""
        bs_pair = input_ids.size(0)
        hidden = self.clip.encode_text(input_ids).float()
        return hidden.view(bs_pair, -1, hidden.size(-1))

    def get_visual_output(self, video, video_mask=None, video_frame=-1):
        """-> ([bs_pair, T_final, D] fp32, cluster_loss)   (clip4clip.py:274-281)"""
        bs_pair = video_mask.size(0)
        hidden, cluster_loss = self.clip.encode_image(video, video_frame=video_frame)
        return hidden.view(bs_pair, -1, hidden.size(-1)).float(), cluster_loss

    def get_video_mask_after_cluster(self, video_mask):
        """Mask of a segment = mask of its last frame (clip4clip.py:436-447)."""
        if self.cluster_algo in ['kmediods++', 'pooling', 'sparse_sampling', 'spectral']:
            # same columns as the reference's arange(f_frame_duration - 1, T, T // final_frames) index, as a strided
            # view: no arange / gather kernels in the step
            return video_mask[:, self.f_frame_duration - 1::video_mask.shape[-1] // self.final_frames]
        return video_mask

    def freeze_cip_layers(self, freeze_layer_num):
        """clip4clip.py:449-471 (main.py:102 calls it with --freeze_layer_num before the optimizer is built; every shipped
        launcher passes 0): parameters of ``clip`` below layer ``freeze_layer_num`` stop requiring a gradient.
          -1      nothing is frozen
          k >= 0  everything under ``clip.`` except the heads (ln_final, text_projection, logit_scale, visual.ln_post,
                  visual.proj) and the blocks with index >= k of either tower - so k = 0 freezes the patch / class / position
                  embeddings, ln_pre and the token embedding; a block's token-cluster module lives under ``...resblocks.N.`` and
                  follows block N.  The seqTransf head is not under ``clip.`` and always trains.
        The training towers then run each tower's frozen prefix on the fused forward and compute no gradient for a frozen
        tensor (centerclip_amd.train)."""
        assert -1 <= freeze_layer_num <= 12
        if freeze_layer_num == -1 or not hasattr(self, "clip"):
            return
        if self.linear_patch == '3d':
            # As the reference behaves, not as its docstring reads: its '3d' exception tests ``name.find("conv2.")`` for truth,
            # and str.find gives -1 (true) for a name without "conv2." and 7 (true) for "visual.conv2.weight" - so with
            # linear_patch '3d' every parameter stays trainable.
            return
        heads = ("ln_final.", "text_projection", "logit_scale", "visual.ln_post.", "visual.proj")
        towers = ("visual.transformer.resblocks.", "transformer.resblocks.")
        for name, param in self.clip.named_parameters():
            if name.startswith(heads):
                continue
            tower = next((t for t in towers if name.startswith(t)), None)
            if tower is not None and int(name[len(tower):].split(".")[0]) >= freeze_layer_num:
                continue
            param.requires_grad = False

    def _loose_similarity(self, sequence_output, visual_output, attention_mask, video_mask):
        """exp(logit_scale) * t_hat @ v_bar^T   (clip4clip.py:324-367).  In training mode the features of all ranks are
        gathered first (:351-355) - one packed RCCL all-gather instead of three + a barrier."""
        sequence_output, visual_output = sequence_output.contiguous(), visual_output.contiguous()
        if self.sim_header == "seqTransf":
            visual_output = self._seq_head_any(visual_output, video_mask)
        if self.training:
            visual_output, video_mask, sequence_output = all_gather(visual_output, video_mask.contiguous(),
                                                                    sequence_output)
        text = sequence_output.squeeze(1)
        scale = self._logit_scale_value()
        if visual_output.ndim == 2:      # already pooled + normalised (eval with pre_visual_pooling, :357)
            L.require_device(text, visual_output)
            return ops.scaled_dot_nt(ops.normalize_rows(text), visual_output, mult=T.logit_multiplier(scale))
        return ops.loose_similarity(text, visual_output, video_mask, scale)

    def get_similarity_logits(self, sequence_output, visual_output, attention_mask, video_mask, shaped=False):
        """-> (logits [Bt, Bv], ())   (clip4clip.py:412-434)"""
        if shaped is False:
            if attention_mask is not None:
                attention_mask = attention_mask.view(-1, attention_mask.shape[-1])
            video_mask = video_mask.view(-1, video_mask.shape[-1])
        if visual_output.ndim == 3 and video_mask.shape[1] != visual_output.shape[1]:
            video_mask = self.get_video_mask_after_cluster(video_mask)
        assert self.sim_header in ["meanP", "seqTransf"]
        logits = self._loose_similarity(sequence_output, visual_output, attention_mask, video_mask)
        if self.camoe_dsl:                       # (clip4clip.py:430-432, over the rows this call was given)
            logits = ops.dual_softmax(logits)
        return logits, ()
