#!/usr/bin/env python3
"""Vocoder server -- MI355X mirror of dual_npu/vocoder_server.py: same protocol (i32 n + i64[n*16] in,
i32 n_samples + i16 out), 64-frame chunks, overlap-16 linear crossfade with the reference's chunk
walk (including its tail-chunk quirk) and its int16 rule, all behind voc_synthesize
(include/qwen3tts_voc.h).

    python -m qwen3_tts_axera_russian_amd.vocoder_server --model qwen3tts_voc.q3w
"""
from __future__ import annotations

import argparse
import os
import signal
import socket
import time

import numpy as np

from . import protocol as P
from .vocoder import Vocoder

SAMPLE_RATE = 24000
SAMPLES_PER_TOKEN = 1920


class VocoderServer:
    def __init__(self, model_path, socket_path="/tmp/qwen3_voc.sock", max_tokens=64, install_signal_handlers=True, max_batch=1):
        self.socket_path = socket_path
        self.voc = Vocoder(model_path, max_tokens, max_batch)
        self.max_tokens = self.voc.chunk_tokens
        print(f"Vocoder: HIP/gfx950 fp32, max_tokens={self.max_tokens}")
        self._running = True
        if install_signal_handlers:
            signal.signal(signal.SIGINT, self._signal_handler)
            signal.signal(signal.SIGTERM, self._signal_handler)

    def _signal_handler(self, signum, frame):
        self._running = False

    def _inference_chunk(self, padded):
        """the model's output tensor for one padded chunk: voc_chunk_samples long (callers slice it numpy-style)"""
        return self.voc.decode(np.asarray(padded).reshape(1, -1))[0]

    def synthesize(self, codes_array):
        """codes [n,16] -> float32 audio (vocoder_server.py:73-121 semantics, chunk walk on the library side)."""
        return self.voc.synthesize(np.asarray(codes_array)[:, :16])

    def synthesize_int16(self, codes_array):
        return self.voc.synthesize(np.asarray(codes_array)[:, :16], int16=True)

    def synthesize_batch(self, codes_list, int16=True):
        """U utterances in one call (voc_synthesize_batch), each what synthesize gives it; 0 frames give an empty array."""
        return self.voc.synthesize_batch([np.asarray(c)[:, :16] for c in codes_list], int16)

    def serve(self):
        if os.path.exists(self.socket_path):
            os.unlink(self.socket_path)
        sock = socket.socket(socket.AF_UNIX, socket.SOCK_STREAM)
        sock.bind(self.socket_path)
        sock.listen(1)
        sock.settimeout(1.0)
        os.chmod(self.socket_path, 0o666)
        print(f"\nVocoder Server listening on {self.socket_path}")
        while self._running:
            try:
                conn, _ = sock.accept()
            except socket.timeout:
                continue
            try:
                codes = P.read_voc_request(conn)
                if codes is not None:
                    t0 = time.time()
                    audio = self.synthesize_int16(codes)
                    print(f"  Vocoder: {len(codes)} tokens -> {len(audio)} samples ({time.time() - t0:.3f}s)")
                    conn.sendall(P.pack_voc_reply(audio))
            except Exception as e:
                print(f"  Vocoder Error: {e}")
            finally:
                conn.close()
        sock.close()
        if os.path.exists(self.socket_path):
            os.unlink(self.socket_path)
        self.voc.close()
        print("Vocoder Server stopped.")


def main():
    ap = argparse.ArgumentParser(description="Qwen3-TTS Vocoder Server (MI355X / HIP)")
    ap.add_argument("--model", required=True, help="Q3TTSW1 container holding voc.*")
    ap.add_argument("--socket", default="/tmp/qwen3_voc.sock")
    a = ap.parse_args()
    VocoderServer(a.model, a.socket).serve()


if __name__ == "__main__":
    main()
