from .episodes import (EpisodeSampler, Graph, cached_graph_pool, connected_graph_pool, device_graph_pool, generate_graph_pool,
                       load_graph_pool, pack_episodes, packed_graph_pool, save_graph_pool, synthetic_graph_pool)
from .vector_env import HipGraphVectorEnv, mpr_sets

__all__ = ["HipGraphVectorEnv", "mpr_sets", "Graph", "EpisodeSampler", "pack_episodes", "synthetic_graph_pool", "packed_graph_pool",
           "save_graph_pool", "load_graph_pool", "cached_graph_pool", "device_graph_pool", "generate_graph_pool",
           "connected_graph_pool"]
