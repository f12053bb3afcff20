"""``python -m birdnet_stm32 <command>`` dispatcher (reference: birdnet_stm32/__main__.py:12-47).

``evaluate``, ``embed`` (embeddings of audio files, this build only), ``analyze`` (per-chunk detections over whole recordings, this build only), ``probe`` (a new classifier head on frozen embeddings, the reference's ``train --linear_probe``), ``search`` (nearest embeddings of query clips, this build only), ``cluster`` (k-means over embed archives, this build only), ``project`` (2-D t-SNE maps of embed archives, this build only), ``density`` (HDBSCAN over embed archives, this build only), ``reduce`` (PCA and whitening of embed archives, this build only), ``propagate`` (a few labels spread over embed archives, this build only), ``select`` (which rows of embed archives to label next, this build only), ``indices`` (acoustic indices of whole recordings, no model, this build only) and ``convert`` (own post-training quantisation, no TensorFlow) exist in this build; the reference's train /
deploy / board-test commands are outside the accelerated path and answer with a pointer to the reference package.
"""

import sys

USAGE = "Usage: birdnet-stm32 {train,convert,evaluate,embed,analyze,probe,search,cluster,project,density,reduce,propagate,select,indices,deploy,board-test}"


def main():
    if len(sys.argv) < 2:
        print(USAGE)
        sys.exit(1)
    command = sys.argv[1]
    sys.argv = [f"birdnet-stm32 {command}"] + sys.argv[2:]
    if command == "evaluate":
        from birdnet_stm32.cli.evaluate import main as run

        run()
    elif command == "embed":
        from birdnet_stm32.cli.embed import main as run

        run()
    elif command == "analyze":
        from birdnet_stm32.cli.analyze import main as run

        run()
    elif command == "probe":
        from birdnet_stm32.cli.probe import main as run

        run()
    elif command == "search":
        from birdnet_stm32.cli.search import main as run

        run()
    elif command == "cluster":
        from birdnet_stm32.cli.cluster import main as run

        run()
    elif command == "project":
        from birdnet_stm32.cli.project import main as run

        run()
    elif command == "density":
        from birdnet_stm32.cli.density import main as run

        run()
    elif command == "reduce":
        from birdnet_stm32.cli.reduce import main as run

        run()
    elif command == "propagate":
        from birdnet_stm32.cli.propagate import main as run

        run()
    elif command == "select":
        from birdnet_stm32.cli.select import main as run

        run()
    elif command == "indices":
        from birdnet_stm32.cli.indices import main as run

        run()
    elif command == "convert":
        from birdnet_stm32.cli.convert import main as run

        run()
    elif command in ("train", "deploy", "board-test"):
        print(f"'{command}' is not part of the MI355X hot-path build; use the reference package for it.")
        sys.exit(2)
    else:
        print(f"Unknown command: {command}")
        print(USAGE)
        sys.exit(1)


if __name__ == "__main__":
    main()
