"""Drop-in for the one piece of ``cuml`` the reference uses: ``cuml.cluster.HDBSCAN`` (GNNEmbedding/
embedding_base.py:40-41).  With ``cuml_shim`` on ``sys.path``, ``from cuml.cluster import HDBSCAN`` binds to the GPU
HDBSCAN of hierarchicalgnn_amd."""
