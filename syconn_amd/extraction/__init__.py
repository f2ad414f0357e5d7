"""Device-side successors of ``syconn.extraction`` stages that consume the dense predictions: object
extraction (``object_extraction_steps``, ``object_extraction_wrapper``), label statistics (``find_object_properties``), contact sites
and synapses (``cs_extraction_steps``) and their agglomeration into cell-level synapses (``cs_processing_steps``)."""
