"""The attribute sample's ratings as a loaded experiment, for the plugin tests."""
import os
import shutil

SAMPLE = os.path.join(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))), "config_files", "attribute_sample")


def experiment(folder, k):
    """The attribute sample's ratings as a loaded experiment: (data, config)."""
    from elliot_amd import run as runner
    os.makedirs(folder / "cfg", exist_ok=True)
    shutil.copy(os.path.join(SAMPLE, "dataset.tsv"), folder / "cfg" / "dataset.tsv")
    exp = {"dataset": "attribute_sample", "data_config": {"strategy": "dataset", "dataset_path": "dataset.tsv"},
           "splitting": {"test_splitting": {"strategy": "random_subsampling", "test_ratio": 0.2}},
           "top_k": k, "evaluation": {"simple_metrics": ["nDCG", "Recall"], "cutoffs": [k, 5]},
           "path_output_rec_result": "out/recs/", "path_output_rec_weight": "out/weights/", "path_output_rec_performance": "out/perf/"}
    cfg = runner.build_config(exp, str(folder / "cfg"))
    return runner.load_data(exp, cfg, str(folder / "cfg")), cfg
