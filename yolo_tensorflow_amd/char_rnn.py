"""Character-level recurrent networks (darknet's examples/rnn.c over rnn.cfg / gru.cfg): a one-hot symbol in, a stack of [rnn] / [gru] / [lstm]
layers, [connected], [softmax], and the sampled symbol fed back -- on the device for a whole generation (hip.Engine.sequence).

    net = CharRNN("rnn.cfg", "shakespeare.weights")
    print(net.generate("The ", 200, temp=0.7, rseed=3).decode(errors="replace"))
    print(net.score(open("held_out.txt", "rb").read())["bpc"])
"""
import ctypes as C
import math
import numpy as np
from . import hip, darknet_io as IO


def _tokens(text):
    """str (latin-1: one symbol per byte, as darknet reads chars), bytes, or a sequence of ints -> int32 [len]"""
    if isinstance(text, str):
        text = text.encode("latin-1")
    if isinstance(text, (bytes, bytearray)):
        return np.frombuffer(bytes(text), dtype=np.uint8).astype(np.int32)
    return np.ascontiguousarray(text, dtype=np.int32).reshape(-1)


class CharRNN:
    """A vector-input network over symbols 0 .. inputs-1.  cfg: cfg text, or the path / shipped name of one; darknet's own cfg (`inputs=256`, no image
    size) gets the [net] key `yolo_input=vector` added.  weights: a .weights path, a flat float32 stream, or None for seeded synthetic ones.
    The engine runs with darknet semantics (batch norm folded with CPU darknet's epsilon), as classifier.py's and the veneer's do: what generate
    and score promise is darknet's arithmetic on darknet's files."""

    # rnn.c:291 compares a float probability with the double .0001: p < .0001 there is p <= 1e-4f in floats, which is p < the next float above it
    CLIP = float(np.nextafter(np.float32(1e-4), np.float32(1)))

    def __init__(self, cfg, weights=None, dtype=hip.BF16, streams=1, device=0):
        text = cfg if "[" in cfg else IO.cfg_text(cfg)
        self.cfg = IO.with_vector_input(text)
        self.engine = hip.Engine(self.cfg, max_batch=streams, dtype=dtype, semantics=hip.SEM_DARKNET, device=device)
        self.inputs = self.engine.vector_inputs
        self.streams = streams
        if isinstance(weights, str):
            self.engine.load_weights(weights)
        else:
            self.engine.set_weights(IO.synth_weights(IO.parse_cfg(self.cfg), seed=0) if weights is None else weights)

    def close(self):
        self.engine.close()

    @staticmethod
    def darknet_uniforms(rseed, count):
        """`count` draws of darknet's rand_uniform(0, 1) -- (float)rand() / RAND_MAX in floats -- from the C library after srand(rseed): what
        sample_array consumes in `darknet rnn generate -srand rseed`, when nothing else draws in between."""
        libc = C.CDLL(None)
        libc.srand(C.c_uint(rseed)); libc.rand.restype = C.c_int
        draws = np.array([libc.rand() for _ in range(count)], dtype=np.int64)
        return (draws.astype(np.float32) / np.float32(2147483647)).astype(np.float32)

    def generate(self, seed, num, temp=0.7, rseed=0, uniforms=None):
        """test_char_rnn (rnn.c:245-297): the states start at zero, every [softmax] runs at `temp`, the seed's symbols are fed in order and `num`
        symbols are sampled, each fed back.  -> the seed followed by the sampled symbols, bytes for a str / bytes seed, else an int32 array.
        `temp` stays the engine's temperature until the next generate(); score() runs at the cfg's own and leaves that behind.  uniforms: the sampler's `num` draws (default: darknet_uniforms(rseed, num))."""
        tok = _tokens(seed)
        if tok.size == 0:
            tok = np.zeros(1, dtype=np.int32)          # rnn.c:262: c = 0
        u = self.darknet_uniforms(rseed, num) if uniforms is None else np.ascontiguousarray(uniforms, dtype=np.float32).reshape(-1)
        if num < 1 or u.size != num:
            raise hip.YoloError("generate: num >= 1 and as many uniforms are needed")
        self.engine.reset_state()
        self.engine.set_temperature(temp)
        out = self.engine.sequence(tok.reshape(-1, 1), tok.size - 1 + num, uniforms=u.reshape(-1, 1), clip=self.CLIP)
        all_tokens = np.concatenate([tok, out.reshape(-1)])
        return bytes(all_tokens.astype(np.uint8).tolist()) if isinstance(seed, (str, bytes, bytearray)) else all_tokens

    def score(self, text, seed=""):
        """valid_char_rnn (rnn.c:435-471): the states start at zero, the seed is fed, then for every symbol of `text` but the last the network's
        probability of the symbol that follows it is read -- one teacher-forced call, the logs summed on the host in the reference's types.
        -> dict(count, words, bpc, perplexity, word_perplexity), the last line the reference prints."""
        pre, tok = _tokens(seed), _tokens(text)
        if tok.size < 2:
            raise hip.YoloError("score: at least two symbols are needed")
        fed = np.concatenate([pre, tok[:-1]]).astype(np.int32)
        self.engine.reset_state()
        self.engine.reset_temperature()          # valid_char_rnn sets none: the cfg's own, whatever an earlier generate() ran at
        _, probs = self.engine.sequence(fed.reshape(-1, 1), fed.size, want_probs=True)
        log2 = np.float32(math.log(2.0))
        total, words = np.float32(0), 1
        for k in range(tok.size - 1):
            nxt = int(tok[k + 1])
            if nxt in (32, 10, 9):
                words += 1
            total = np.float32(float(total) + math.log(float(probs[pre.size + k, 0, nxt])) / float(log2)) if probs[pre.size + k, 0, nxt] > 0 else np.float32(-np.inf)
        count = tok.size - 1
        return dict(count=count, words=words, bpc=float(-total / count), perplexity=float(2.0 ** (-float(total) / count)), word_perplexity=float(2.0 ** (-float(total) / words)))
