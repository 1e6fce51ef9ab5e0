"""CPU: the record of what sequence 0's KV cache holds and the common prefix with a new prompt (omchat_amd/prefix.py; DESIGN.md
section 12), and the refusals of generate(reuse_cache=True) that need no GPU."""
import pytest

from omchat_amd import prefix as px

NTOK = 4


def _slots(ids, keys):
    return px.slots_from_ids(ids, NTOK, keys)


def test_identical_prompts_keep_all_but_one():
    a = _slots([3, -200, 17, 18], [7])
    assert len(a) == 3 + NTOK
    assert px.common_prefix(a, a) == len(a)
    assert px.keep_count(a, a) == len(a) - 1                      # one row must be prefilled to have logits
    assert px.keep_count(a, a, cached=5) == 5                     # never more than the cache holds


def test_changed_token():
    a = _slots([3, -200, 17, 18, 19], [7])
    b = _slots([3, -200, 17, 99, 19], [7])
    assert px.common_prefix(a, b) == 1 + NTOK + 1
    assert px.keep_count(a, b) == 1 + NTOK + 1


def test_changed_tile_in_the_middle_ends_at_its_first_row():
    a = _slots([3, -200, 17, -200, 18, -200, 19], [10, 11, 12])
    b = _slots([3, -200, 17, -200, 18, -200, 19], [10, 99, 12])
    assert px.common_prefix(a, b) == 1 + NTOK + 1
    # rows of one tile differ from each other: the same key at another row is no match
    assert (10, 0) != (10, 1) and a[1] == (10, 0) and a[NTOK] == (10, NTOK - 1)


def test_same_tile_content_under_another_index():
    # turn 1: tiles [A, B]; turn 2 passes [B, A] and swaps the sentinels' meaning: keys follow content, so the prefix follows content
    a = _slots([3, -200, -200], [10, 11])
    b = _slots([3, -200, -200], [11, 10])
    assert px.common_prefix(a, b) == 1
    # the same content listed at index 1 instead of 0 with one more (unused) tile in front of the list is still a match by key
    c = px.slots_from_plan([3] + [-1 - (1 * NTOK + r) for r in range(NTOK)], NTOK, [55, 10])
    assert px.common_prefix(a, c) == 1 + NTOK


def test_record_with_generated_ids():
    prompt = _slots([3, -200, 17], [7])
    gen = [40, 41, 42, 43]
    # four ids emitted, three cached (the last emitted id never is)
    rec = px.extend_record(prompt, gen, cached=len(prompt) + 3)
    assert rec == prompt + [40, 41, 42]
    turn2 = _slots([3, -200, 17, 40, 41, 42, 43, 50, 51], [7])
    assert px.common_prefix(rec, turn2) == len(prompt) + 3
    assert px.keep_count(rec, turn2, cached=len(rec)) == len(rec)
    # a cache trimmed below the prompt (kv_rewind) trims the record
    assert px.extend_record(prompt, gen, cached=2) == prompt[:2]
    # the model answered differently this time
    other = _slots([3, -200, 17, 40, 77], [7])
    assert px.common_prefix(rec, other) == len(prompt) + 1


def test_empty_record_and_empty_prompt():
    a = _slots([3, 4], [])
    assert px.common_prefix(None, a) == 0 and px.common_prefix([], a) == 0
    assert px.keep_count(None, a) == 0
    assert px.keep_count(a, []) == 0


def test_sentinel_handling():
    assert _slots([-200], [5]) == [(5, r) for r in range(NTOK)]
    with pytest.raises(ValueError):
        _slots([-200, -200], [5])                                  # more sentinels than tiles
    plan = [3, -1, -2, -3, -4, 9]
    assert px.slots_from_plan(plan, NTOK, [5]) == _slots([3, -200, 9], [5])
    with pytest.raises(ValueError):
        px.slots_from_plan([3, px.PAD_ROW], NTOK, [])
    # a token id never equals a feature row
    assert px.common_prefix([0], [(0, 0)]) == 0


def test_reuse_refusals():
    px.check_reuse_args(1, 1, None)
    px.check_reuse_args(1, 1, [[1, 1, 1]])
    with pytest.raises(ValueError, match="batch size"):
        px.check_reuse_args(2, 1)
    with pytest.raises(ValueError, match="num_beams"):
        px.check_reuse_args(1, 4)
    with pytest.raises(ValueError, match="padded"):
        px.check_reuse_args(1, 1, [[1, 1, 0]])
    with pytest.raises(ValueError, match="right padding"):
        px.check_reuse_args(1, 1, None, "left")


def test_generate_refuses_before_touching_the_engine():
    """generate(reuse_cache=True) with b > 1, beams or a padded batch raises before any engine call: an engine that fails on every
    attribute access proves it"""
    import torch
    from omchat_amd.model.omchat_qwen2 import OmChatQwen2ForCausalLM, _GenerationConfig

    class Boom:
        def __getattr__(self, name):
            raise AssertionError(f"engine touched: {name}")

    m = OmChatQwen2ForCausalLM.__new__(OmChatQwen2ForCausalLM)
    m.engine = Boom()
    m.config = type("C", (), {})()
    m.generation_config = _GenerationConfig(do_sample=False, num_beams=1, reuse_cache=True, max_new_tokens=4, eos_token_id=None,
                                            pad_token_id=None)
    with pytest.raises(ValueError, match="batch size"):
        m.generate(torch.tensor([[1, 2], [3, 4]]))                # read from generation_config
    with pytest.raises(ValueError, match="num_beams"):
        m.generate(torch.tensor([[1, 2]]), num_beams=2, reuse_cache=True)
    with pytest.raises(ValueError, match="padded"):
        m.generate(torch.tensor([[1, 2]]), attention_mask=torch.tensor([[0, 1]]), reuse_cache=True)
