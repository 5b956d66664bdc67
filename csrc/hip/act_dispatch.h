// Activation-dtype dispatch of the launchers: runs the statement once with
// act_t bound to the type the flag names (0 = fp32, 1 = bf16, 2 = fp16).
// `bf16` and `fp16` are the aliases of the including .hip file.
#ifndef PCNN_ACT_DISPATCH_H
#define PCNN_ACT_DISPATCH_H

#define PCNN_DISPATCH(flag, ...)                    \
  do {                                               \
    if ((flag) == 1) {                               \
      using act_t = bf16;                            \
      __VA_ARGS__;                                   \
    } else if ((flag) == 2) {                        \
      using act_t = fp16;                            \
      __VA_ARGS__;                                   \
    } else {                                         \
      using act_t = float;                           \
      __VA_ARGS__;                                   \
    }                                                \
  } while (0)

#endif  // PCNN_ACT_DISPATCH_H
