"""Host side of teacher-forced scoring: the label half of prepare_inputs_labels_for_multimodal
(omchat_arch.py:112-199) on top of the splice plan, and the shift of Qwen2ForCausalLM's loss.  Integers only, no device."""
import torch

from .constants import IMAGE_TOKEN_INDEX

IGNORE_INDEX = -100          # omchat/constants.py


def splice_labels(src_index, input_ids, attention_mask, labels):
    """The reference's `new_labels` [b, S] (int64, CPU).  src_index int32 [b, S] is the splice plan of the same call (>= 0: a token slot,
    < 0: a feature row or padding).  A row's labels are filtered by its attention mask and lose the image-token positions
    (omchat_arch.py:116, :133-137); what is left fills the row's token slots in order -- fewer slots than labels when
    tokenizer_model_max_length cut the row (:164).  Feature rows (:152), padding on either side (:170) and everything beyond the cut
    are IGNORE_INDEX."""
    idx = src_index.detach().to("cpu")
    ids = input_ids.detach().to("cpu", torch.int64)
    lab = labels.detach().to("cpu", torch.int64)
    if lab.shape != ids.shape:
        raise ValueError(f"labels {tuple(lab.shape)} must have the shape of input_ids {tuple(ids.shape)}")
    keep = ids.ne(IMAGE_TOKEN_INDEX)
    if attention_mask is not None:
        keep &= attention_mask.detach().to("cpu").ne(0)
    out = torch.full(tuple(idx.shape), IGNORE_INDEX, dtype=torch.int64)
    for i in range(idx.shape[0]):
        slots = torch.nonzero(idx[i] >= 0).flatten()
        out[i, slots] = lab[i][keep[i]][:slots.numel()]
    return out


def shift_labels(new_labels):
    """shift[:, t] = new_labels[:, t + 1], last column IGNORE_INDEX: slot t's row predicts the label of slot t + 1 (Qwen2ForCausalLM.forward:
    logits[..., :-1, :] against labels[..., 1:])"""
    out = torch.full_like(new_labels, IGNORE_INDEX)
    out[:, :-1] = new_labels[:, 1:]
    return out


def check_labels(labels, vocab):
    """a label is IGNORE_INDEX or a token id: anything else is refused before a launch (torch's cross_entropy raises on it too)"""
    bad = labels.ne(IGNORE_INDEX) & ((labels < 0) | (labels >= vocab))
    if bool(bad.any()):
        raise ValueError(f"labels must be {IGNORE_INDEX} or token ids in [0, {vocab}): got {int(labels[bad][0])}")
