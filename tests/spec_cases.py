"""Shared by tests/test_spec_decode_{cpu,gpu}.py: the verify-attention probe cases (arguments of
attn_edges.paged_case, seed 7) and scripted proposers.  Plain helpers: no fixtures, no pytest settings."""

SPEC_CASES = {
    # no cached context, drafts across a block edge, a single row, a full tile, many blocks
    "spec_d128_g4": dict(D=128, Hq=8, Hkv=2, kv_lens=[5, 66, 64, 200, 577], q_lens=[5, 5, 1, 8, 3]),
    # 64 rows per KV head
    "spec_d128_g8": dict(D=128, Hq=8, Hkv=1, kv_lens=[130, 1030], q_lens=[8, 8]),
    "spec_d64_g2": dict(D=64, Hq=4, Hkv=2, kv_lens=[70, 9, 300], q_lens=[6, 8, 2]),
}

VOCAB = 512   # LlamaConfig.tiny()


class Wrong:
    """Always-wrong drafts (up to a 1-in-512 accident per token, which only costs nothing): successors of the last
    token, which the random-weight tiny model has no reason to produce."""

    def propose(self, tokens, k):
        return [(tokens[-1] + 1 + i) % VOCAB for i in range(k)]


class Replay:
    """Drafts from recorded outputs: the sequence is recognised by its prompt (a preempted sequence still starts with
    it), the draft is what the recording holds behind the tokens generated so far.  ``right``: only the first
    ``right`` drafts of a proposal are the recording's, the rest are off by one."""

    def __init__(self, prompts, outputs, right=None):
        self.known = [(list(p), list(o)) for p, o in zip(prompts, outputs)]
        self.right = right

    def propose(self, tokens, k):
        for p, o in self.known:
            if tokens[:len(p)] == p and tokens[len(p):] == o[:len(tokens) - len(p)]:
                d = o[len(tokens) - len(p):len(tokens) - len(p) + k]
                if self.right is not None:
                    d = [t if i < self.right else (t + 1) % VOCAB for i, t in enumerate(d)]
                return d
        return []
