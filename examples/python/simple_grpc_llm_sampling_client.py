#!/usr/bin/env python3
"""LLM token streaming with per-request sampling: one greedy request,
then the same sampled request twice with one seed (temperature, top_k,
top_p and seed are optional inputs of the generate models; the same
seed reproduces the same tokens). Needs a server with ``llama_tiny``."""
import argparse
import queue

import numpy as np

import tritonclient.grpc as grpcclient


def stream_tokens(client, results, model, prompt, max_tokens, sampling=None):
    inputs = [
        grpcclient.InferInput("input_ids", [len(prompt)], "INT64"),
        grpcclient.InferInput("max_tokens", [1], "INT32"),
    ]
    inputs[0].set_data_from_numpy(np.asarray(prompt, dtype=np.int64))
    inputs[1].set_data_from_numpy(np.array([max_tokens], dtype=np.int32))
    types = {"temperature": ("FP32", np.float32), "top_k": ("INT32", np.int32),
             "top_p": ("FP32", np.float32), "seed": ("UINT64", np.uint64)}
    for name, value in (sampling or {}).items():
        datatype, npdt = types[name]
        inp = grpcclient.InferInput(name, [1], datatype)
        inp.set_data_from_numpy(np.array([value], dtype=npdt))
        inputs.append(inp)
    client.async_stream_infer(model, inputs, enable_empty_final_response=True)
    tokens = []
    while True:
        result, error = results.get(timeout=60)
        assert error is None, error
        if result.is_final_response():
            return tokens
        tokens.append(int(result.as_numpy("token_id")[0]))


if __name__ == "__main__":
    parser = argparse.ArgumentParser()
    parser.add_argument("-u", "--url", default="127.0.0.1:8001")
    parser.add_argument("-m", "--model-name", default="llama_tiny")
    parser.add_argument("-n", "--max-tokens", type=int, default=12)
    args = parser.parse_args()

    prompt = [3, 14, 15, 92, 65, 35, 89, 79]
    sampling = {"temperature": 0.9, "top_k": 40, "top_p": 0.95, "seed": 1234}
    with grpcclient.InferenceServerClient(args.url) as client:
        results = queue.Queue()
        client.start_stream(
            callback=lambda result, error: results.put((result, error)))
        greedy = stream_tokens(client, results, args.model_name, prompt,
                               args.max_tokens)
        first = stream_tokens(client, results, args.model_name, prompt,
                              args.max_tokens, sampling)
        second = stream_tokens(client, results, args.model_name, prompt,
                               args.max_tokens, sampling)
        client.stop_stream()
    print("greedy :", greedy)
    print("sampled:", first)
    print("sampled:", second)
    assert len(greedy) == len(first) == args.max_tokens
    assert first == second, "the same seed must reproduce the same tokens"
    print("PASS: llm sampling")
