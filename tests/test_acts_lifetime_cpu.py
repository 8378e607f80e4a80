"""CPU: an activation set that Tagger.acts evicts gives its buffers back when the last reference goes, without waiting for the
garbage collector -- at the benchmark's shapes a set holds > 100 GB, and a reference cycle between the set and its per-layer views
(engine._LayerView) kept evicted sets alive until the device was full."""
import gc
import weakref

from kbner import engine


def test_an_activation_set_is_freed_by_its_last_reference():
    cfg = engine.EncoderConfig(vocab_size=64, hidden_size=128, num_hidden_layers=2, num_attention_heads=2, intermediate_size=256,
                               max_position_embeddings=18)
    gc.disable()
    try:
        ac = engine._Acts(cfg, 2, 16, "cpu", 0)
        ac.drop_buffers()
        assert len(ac.layers) == 2 and ac.layers[1].xres is ac.layers[0].xo and ac.layers[0].dhm is ac.dhm[0]
        gone = weakref.ref(ac)
        buf = weakref.ref(ac.layers[0].h1)
        del ac
        assert gone() is None and buf() is None
    finally:
        gc.enable()
