"""Development settings: alternative forms of the host path that exist for A/B measurements and for the parity tests.

None of these is an environment switch.  Every default is the measured-fastest form (DESIGN.md sections 6, 8, 9 carry the
figures); a test or a tool under ``tools/`` changes an attribute here (``monkeypatch.setattr(_dev, "ATOM_AHEAD", False)``)
to run the other form against the same fixtures; every module reads these attributes at CALL time (none copies one
into a module global at import), so a change made after the package was imported takes effect.  What a switch selects
travels by value from there on: the atom level issued ahead is the handle ``start_atom_level`` returns, "beside the atom
level" is the encoder's ``beside=`` argument.  The runtime switches a user of the package sees are the few in
README.md; the compile-time tuning switches of the kernels live in the ``dev`` variant of the library
(``python -m ggpm_amd.build --variant dev -DGGPM_DEV_SWITCHES``, csrc/common.h: ggpm_dev_env).
"""

# ---- the teacher-forced decoder (decoder.py, atom_decode.py, tree_decode.py; reference ggpm/decoder.py:166-284)
DECODER_BATCHED = True     # tree-side levels as ONE level call each over the decode-time DAG (False: the reference's step loop)
ATOM_DECODE = True         # atom level as one autograd node on host-built index tables (False: through IncMPNEncoder per step)
ATOM_AHEAD = True          # ... issued on its own stream BEFORE the encoder, joined where the attachment level needs it
ATOM_PRIORITY = True       # ... on a high-priority stream
ATOM_ASYNC = True          # ... its two step loops (one C call each, csrc/decode.hip) issued by a worker thread of the library
                           # (ggpm_decode_steps_*_async; False: by the calling thread)
TREE_COMPOSITE = True      # each tree-side decoder level as one autograd node (False: op by op)
TREE_DRIVER = True         # ... whose two directions are one C call each (csrc/tree_level.hip; False: ~30 ctypes calls)
HEADS_COMPOSITE = True     # the four score heads + losses + accuracies as ONE autograd node (heads_fused.py; False: ~30 nodes)
TREE_WGRADS_ASIDE = True   # ... and whose parameter gradients are formed on the second stream, beside the rest of the backward
ENC_NARROW = True          # the encoder's levels take two row tiles per workgroup while they run beside the atom-level chain
                           # ("fwd" / "bwd": in that direction only)

# ---- forward-only forms (fused.py)
FORWARD_ONLY = True        # a call autograd will not record (grad mode off, or nothing it reads requires grad) runs the
                           # forward-only form: no stashes, no backward-only layout (False: the training forward, for A/B)

# ---- gradients (functional.py, parallel.py, optim.py)
DEFER_EARLY = True         # deferred weight-gradient contractions start beside the atom level's backward (second stream)
INDEX_MEMO = True          # CSRs / transposes / masks derived from RESIDENT index tensors are remembered on them
RECORD_GRADS = False       # published gradients are marked with record_stream(main) (an event record each when released)
GRAD_SINK = True           # the encoder's backward writes its gradients straight into FlatGradSync's flat buffer
HIP_ADAM = True            # FlatAdam's update as one ggpm_adam_step launch (False: torch's fused Adam)

# ---- metrics (property_vae.py)
METRICS_ASYNC = True       # the metrics' copy to pinned memory is enqueued behind the forward and read through its event
