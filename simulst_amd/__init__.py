"""The modules are imported by name (simulst_amd.model, simulst_amd.agent, ...); importing the package loads none of them.
The transducer's simultaneous agents are also reachable from here, on first use."""

_LAZY = {"TransducerAgent": "transducer_agent", "BatchedTransducerStreamingAgent": "transducer_agent", "emit_delays": "transducer_agent"}


def __getattr__(name):
    if name in _LAZY:
        from importlib import import_module
        return getattr(import_module(f".{_LAZY[name]}", __name__), name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
