function [R, taps] = corrFunction(fileNameStr, trackResults, channel, settings, taps, epochs)
% The correlation function along tracked channels: an open-loop replay of tracked
% epochs at any set of tap offsets, on the GPU (bds_mex('corr_function', ...) ->
% bds_corr_function of libbds_mi355x.so).  Beyond the reference, whose loops return
% the Early / Prompt / Late sums at -+settings.dllCorrelatorSpacing only.
%
%   R = corrFunction(fileName, trackResults, channel, settings)
%   R = corrFunction(fileName, trackResults, channel, settings, taps, epochs)
%
% taps    offsets in primary-code chips, the unit of dllCorrelatorSpacing
%         (default -1.6:0.05:1.6; at most 128, |tau| <= 16)
% epochs  1-based epochs of every live channel (default: all of trackResults)
% R       complex [numel(taps) x nComp x numel(epochs) x nChannels], I + 1i*Q of the
%         raw sums; component 1 data, 2 the pilot (when it is tracked), 3 the pilot
%         BOC(6,1) (wide-band mode).  Figure 300 shows |R(tau)| averaged over the
%         chosen epochs, one line per channel and component.
if nargin < 5 || isempty(taps),   taps = -1.6:0.05:1.6; end
live = find([channel.PRN] ~= 0);
if nargin < 6 || isempty(epochs), epochs = 1:numel(trackResults(live(1)).absoluteSample); end

% the NCO state each epoch was correlated with: all five are the epoch's own entries
% (codeFreq and carrFreq are stored before the loop filters replace them,
% tracking.m:361-363,387-389; WB_tracking.m:404-406,428-430)
nE = numel(epochs);
prn = zeros(1, nE * numel(live));
state6 = zeros(6, nE * numel(live));
k = 0;
for c = live
    r = trackResults(c);
    for e = epochs(:).'
        if ~isfinite(r.carrFreq(e)), error('channel %d did not complete epoch %d', c, e); end
        k = k + 1;
        step = r.codeFreq(e) / settings.samplingFreq;
        blksize = ceil((settings.codeLength - r.remCodePhase(e)) / step);
        prn(k) = channel(c).PRN;
        state6(:, k) = [r.absoluteSample(e); blksize; r.remCodePhase(e); r.codeFreq(e); r.remCarrPhase(e); r.carrFreq(e)];
    end
end

p = bds_mex('corr_function', fileNameStr, settings, prn, state6, taps(:).');
nC = p.n_comp;
R = reshape(complex(p.I, p.Q), numel(taps), nC, nE, numel(live));

names = {'data', 'pilot', 'pilot BOC(6,1)'};
figure(300); clf(300); hold on;
lbl = cell(1, 0);
for c = 1:numel(live)
    for m = 1:nC
        plot(taps(:), mean(abs(R(:, m, :, c)), 3));
        lbl{end + 1} = sprintf('PRN %d %s', channel(live(c)).PRN, names{m}); %#ok<AGROW>
    end
end
hold off; grid on; legend(lbl{:});
xlabel('\tau (chips)'); ylabel('|R(\tau)|');
title(sprintf('Correlation function, mean of %d epochs', nE));
end
